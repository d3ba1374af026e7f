"""The whole controller loop of INTEGRATION.md 2 - 2l on ONE engine handle, cycle after cycle, against the composed reference of
tests/loop_case.py: gate -> order from the ledger -> cycle -> commit checks -> run limits with the codes as skip -> boundary ->
releases -> probes, over queues that grow past a workgroup, shrink to less than half, become empty and grow again.

Every call is fed by what the DEVICE answered in the step before (the survivors of its gate, its order, its codes, its admitted jobs,
its `found`, its tables), packed with the packers the reference used; every answer is compared with the cycle's record for equality:
placements, fp64 costs by bit pattern, time maps, ledger and columns, accounting records without their padding word.  A failure names
the cycle and the step, and with them the hand-off that fed it."""
import numpy as np
import pytest

from cranesched_amd import abi
from cranesched_amd.engine import EngineError
from tests import gate_case
from tests import gate_pyref
from tests import helpers
from tests import loop_case as lc
from tests import running_attrs_pyref as rap
from tests import running_pyref as rp
from tests import usage_pyref as up

pytestmark = pytest.mark.gpu
SEED = 1
TL_FIELDS = ("t", "cpu_raw", "mem", "core_lo", "core_hi", "gres", "core_w2", "core_w3")


@pytest.fixture(scope="module")
def plain(built):
    return lc.scenario(SEED)


@pytest.fixture(scope="module")
def preempting(built):
    return lc.scenario(SEED, preempt=True)


class Loop:
    """One engine and the loop's state as the DEVICE left it.  hook(loop, i, step) is called in front of every step ("a" .. "h") and
    behind the last one ("end"); the calls a subclass may wrap are methods of their own (order_call, commit_call, advance_call, release_call)."""

    def __init__(self, eng, scen, preempt=False, hook=None):
        self.eng, self.preempt, self.hook = eng, preempt, hook
        self.U, self.resv, self.first, self.first_tables, self.cycles = scen
        self.trace = []

    def seed(self):
        e = self.eng
        e.set_nodes(self.U.cluster)
        e.set_reservations(self.resv)
        run, ids = self.first.ledger.arrays()
        e.seed_running(run, ids, attrs=rap.to_abi(self.first.columns()))
        self.state = self.first_tables
        self.preempting = []
        self.ledger = e.running_ledger()
        assert rp.same_ledger(self.ledger, self.first.ledger.arrays()) is None, "seed: the device ledger differs from the first ledger"

    def run(self):
        self.seed()
        for i, c in enumerate(self.cycles):
            for step in lc.STEPS + ("end",):
                if self.hook is not None:
                    self.hook(self, i, step)
                if step != "end":
                    getattr(self, "step_" + step)(i, c)
        return self.trace

    def keep(self, *arrays):
        self.trace.append(b"".join(np.ascontiguousarray(a).tobytes() for a in arrays))

    # ---- a ------------------------------------------------------------------------------------------------------------------------
    def step_a(self, i, c):
        tag = f"cycle {i}, step a (gate_pending)"
        if c.arrivals:     # the submissions since the last cycle, on the host (2k: the tables go through host memory)
            self.state = up.apply(self.U.meta, self.state, abi.USAGE_CHARGE, self.U.submit_rows(c.arrivals))[0]
        code, pending, ready, erased, counts, stats = self.eng.gate_pending(c.now, c.gate_jobs, gate_case.pack_events(c.gate_events))
        g = c.gate
        assert np.array_equal(code, g.code), f"{tag}: codes differ at {np.flatnonzero(code != g.code)[:8]}"
        assert np.array_equal(pending, g.pending), f"{tag}: the pending rows differ"
        assert np.array_equal(ready, g.ready_sec) and np.array_equal(erased, c.dep_erased), f"{tag}: ready times or erased entries differ"
        assert np.array_equal(counts, g.counts) and np.array_equal(stats, g.ev_stats), f"{tag}: counts {counts} / {g.counts}, events {stats} / {g.ev_stats}"
        self.gate_code = code
        self.survivors = [c.pending_ids[r] for r in pending]
        self.keep(code, pending, ready, erased, counts, stats)

    # ---- b ------------------------------------------------------------------------------------------------------------------------
    def order_call(self, c, pd):
        return self.eng.priority_order_resident(c.now, lc.CFG, lc.ACCOUNTS, pd)

    def step_b(self, i, c):
        tag = f"cycle {i}, step b (priority_order_resident on the gate's survivors and the ledger of boundary {i - 1})"
        assert self.survivors == c.survivors, f"{tag}: the survivors handed over by step a differ"
        order, prio, n = self.order_call(c, self.U.prio_pending(self.survivors))
        assert n == len(c.order) and np.array_equal(order, c.order), f"{tag}: the order differs"
        assert np.array_equal(prio.view(np.uint64), c.priority.view(np.uint64)), f"{tag}: the priorities differ in their bits"
        self.queue = [self.survivors[k] for k in order]
        self.prio = prio[order]
        self.keep(order, prio)

    # ---- c ------------------------------------------------------------------------------------------------------------------------
    def step_c(self, i, c):
        tag = f"cycle {i}, step c ({'node_select_preempt_resident' if self.preempt else 'node_select'} on the queue in step b's order)"
        assert self.queue == c.queue_ids, f"{tag}: the queue handed over by step b differs"
        self.jobs = jobs = self.U.jobs(self.queue)
        self.po = None
        if self.preempt:
            pre = self.U.preempt(self.queue, self.prio, None, self.preempting)
            pl, po = self.eng.node_select_preempt_resident(c.now, jobs, pre, from_attrs=True)
            d = pl.diff(c.oracle.placements)
            assert d is None, f"{tag}: placements differ from the oracle at {d}"
            assert po.lists() == c.lists, f"{tag}: the preempted lists differ"
            assert po.cancelled_ids() == c.cancelled, f"{tag}: cancelled {po.cancelled_ids()} / {c.cancelled}"
            assert po.preempting_ids() == c.preempting_out, f"{tag}: the preempting set {po.preempting_ids()} / {c.preempting_out}"
            assert np.array_equal(self.eng.costs().view(np.uint64), c.oracle.costs().view(np.uint64)), f"{tag}: fp64 costs differ"
            self.po, self.cancelled = po, po.cancelled_ids()
            self.keep(po.offsets, po.preempted[:int(po.offsets[jobs.num_jobs])], np.array(self.cancelled + [0] + po.preempting_ids(), np.uint32))
        else:
            pl = self.eng.node_select(c.now, jobs)
            helpers.assert_same(self.eng, pl, c.oracle, self.U.cluster, sample_nodes=8, tag=tag)
            self.cancelled = []
        for n, want in c.timelines.items():
            got = self.eng.timeline(n)
            for f in TL_FIELDS:
                assert np.array_equal(got[f], want[f]), f"{tag}: time map of node {n} differs in {f}"
        self.pl = pl
        J = jobs.num_jobs
        self.keep(pl.start_sec[:J], pl.reason[:J], *[getattr(pl, f)[:int(pl.place_offsets[J])] for f in ("node_idx", "ntasks", "cpu_raw", "mem", "core_lo", "core_hi", "gres")],
                  self.eng.costs())

    # ---- d ------------------------------------------------------------------------------------------------------------------------
    def commit_call(self, c):
        return self.eng.commit_check(c.commit_events, self.U.commit_jobs(self.jobs, c.gone, self.po, len(self.ledger[1])))

    def step_d(self, i, c):
        tag = f"cycle {i}, step d (commit_check on the results of step c)"
        code, counts = self.commit_call(c)
        assert np.array_equal(code, c.code), f"{tag}: codes differ at {np.flatnonzero(code != c.code)[:8]}"
        assert np.array_equal(counts, c.counts), f"{tag}: counts {counts} / {c.counts}"
        self.code = code
        self.keep(code, counts)

    # ---- e ------------------------------------------------------------------------------------------------------------------------
    def skip_of(self, code):
        return (code != abi.COMMIT_OK).astype(np.uint8)

    def step_e(self, i, c):
        tag = f"cycle {i}, step e (run limits on step c's results, step d's codes as skip, the tables of release {i - 1})"
        bad = self.state.differences(c.tables_in)
        assert not bad, f"{tag}: the tables handed over by step g and the submissions differ in {bad}"
        self.eng.set_run_limits(self.U.limit_tables(self.state))
        reason, adm = self.eng.apply_run_limits(self.U.limit_jobs(self.queue, self.jobs, self.skip_of(self.code)))
        usage = self.eng.usage()
        assert np.array_equal(reason, c.limit_reason), f"{tag}: reasons differ at {np.flatnonzero(reason != c.limit_reason)[:8]}"
        assert adm == c.admitted, f"{tag}: {adm} admitted, {c.admitted} expected"
        for f in usage.__dataclass_fields__:
            assert np.array_equal(getattr(usage, f), getattr(c.usage, f)), f"{tag}: usage table {f} differs"
        self.limit_reason = reason
        self.state = self.U.with_usage(self.state, usage)
        self.keep(reason, *[getattr(usage, f) for f in usage.__dataclass_fields__])

    # ---- f ------------------------------------------------------------------------------------------------------------------------
    def admit_of(self, reason):
        return (reason == 0).astype(np.uint8)

    def advance_call(self, c, retire, admit):
        if self.jobs.num_jobs == 0:
            return self.eng.advance_running(retire, attrs=True)
        return self.eng.advance_running(retire, c.now, np.array(self.queue, np.uint32), admit, reservation=self.jobs.reservation,
                                        attrs=rap.to_abi(self.U.queue_attrs(self.queue)))

    def step_f(self, i, c):
        tag = f"cycle {i}, step f (advance_running: admit = admitted by step e, retire = what ended before the next now)"
        run, ids = self.ledger
        retire = [int(x) for x, end in zip(ids, run.end_sec) if end <= c.next_now]
        if c.next_now - c.now > 1:
            retire += [x for x in self.cancelled if x not in retire] + [77]
        assert retire == [int(x) for x in c.retire], f"{tag}: the ids to retire, from the device's ledger, differ"
        admit = self.admit_of(self.limit_reason)
        found, nret, nadm = self.advance_call(c, retire, admit)
        assert np.array_equal(found, c.found) and (nret, nadm) == (c.num_retired, c.num_admitted), \
            f"{tag}: found {found} / {c.found}, retired {nret} / {c.num_retired}, admitted {nadm} / {c.num_admitted}"
        self.ledger_before, self.ledger = self.ledger, self.eng.running_ledger()
        f = rp.same_ledger(self.ledger, c.after.ledger.arrays())
        assert f is None, f"{tag}: the device ledger differs from AttrLedger in {f}"
        cols = self.eng.running_attrs()
        f = rap.same_attrs(cols, c.after)
        assert f is None, f"{tag}: running_attrs() differs from AttrLedger in {f}"
        self.released = [x for x, hit in zip(retire, found) if hit]
        self.preempting = self.po.preempting_ids() if self.po is not None else []
        self.keep(found, self.ledger[1], *[getattr(self.ledger[0], x) for x in rp.RUN_FIELDS], *[cols[x] for x in rap.COLUMNS + rap.DERIVED])

    # ---- g ------------------------------------------------------------------------------------------------------------------------
    def release_call(self, rows):
        return self.eng.release_usage(rows)

    def step_g(self, i, c):
        tag = f"cycle {i}, step g (release_usage for the rows step f retired, on the tables step e left)"
        left = [self.queue[j] for j in range(self.jobs.num_jobs) if c.gone[j]]
        left += [c.pending_ids[r] for r in np.flatnonzero(self.gate_code == gate_pyref.DEPENDENCY_NEVER)]
        assert self.released == c.release_ids and left == c.left_ids, f"{tag}: the rows to release differ"
        if not self.released and not left:
            return
        rows = self.U.release_rows(rp.Ledger.from_running(*self.ledger_before), self.released, left)
        self.eng.set_usage_tables(self.U.usage_tables(self.state))
        nf, of, clean = self.release_call(rows)
        got = self.eng.usage_tables()
        assert np.array_equal(nf, c.not_found) and np.array_equal(of, c.over_free), f"{tag}: the not_found / over_free masks differ"
        assert clean == int(((c.not_found == 0) & (c.over_free == 0)).sum()), f"{tag}: num_clean {clean}"
        bad = got.differences(c.tables_out)
        assert not bad, f"{tag}: the tables differ from usage_pyref in {bad}"
        self.state = got
        self.keep(nf, of)
        for f in got.__dataclass_fields__:       # (a record without its padding word)
            a = getattr(got, f)
            self.keep(*([a[n] for n in a.dtype.names if n != "reserved0"] if a.dtype.names else [a]))

    # ---- h ------------------------------------------------------------------------------------------------------------------------
    def step_h(self, i, c):
        tag = f"cycle {i}, step h (probe against the final state of step c)"
        if c.probes is None:
            return
        got = self.eng.probe(c.probes)
        d = got.diff(c.probe_expected)
        assert d is None, f"{tag}: the probes differ from probe_case.expected at {d}"
        Q = c.probes.num_jobs
        self.keep(got.start_sec[:Q], got.reason[:Q], got.node_idx[:int(got.place_offsets[Q])])


def _run(cls, scen, preempt=False, hook=None, loop=Loop):
    eng = cls(device=0)
    try:
        return loop(eng, scen, preempt, hook).run()
    finally:
        eng.close()


# ---- the loop -----------------------------------------------------------------------------------------------------------------------
def test_loop_on_one_handle(engine_cls, plain):
    """Steps a - h for every cycle on one engine, once per selection kernel."""
    assert len(_run(engine_cls, plain)) > 6 * len(plain[4])


def test_loop_with_preemption(engine_default, preempting):
    """The same with the cycle that preempts from the ledger's columns: the preempted lists, the cancelled ids (retired at the boundary)
    and the preempting set handed to the next cycle; a job that waits for its victims is neither admitted by (e) nor by (f)."""
    _run(engine_default, preempting, preempt=True)


def test_two_loops_agree(engine_default, plain):
    """The scenario twice on the same handle, with a fresh seed_running(attrs=) and fresh tables in between: identical bytes the second
    time — no buffer keeps anything of the first run."""
    eng = engine_default(device=0)
    try:
        a = Loop(eng, plain).run()
        b = Loop(eng, plain).run()
        assert len(a) == len(b) and [x == y for x, y in zip(a, b)].count(False) == 0
    finally:
        eng.close()


# ---- foreign calls ------------------------------------------------------------------------------------------------------------------
class Foreign:
    """Independent calls and their references, computed once.  needs_run: served only behind a cycle of the loop's own."""

    def __init__(self, scen):
        from tests import resvq_case, resvq_pyref, submit_case, submit_pyref, valid_pyref
        self.U, self.cycles = scen[0], scen[4]
        U = self.U
        self.valid = valid_pyref.check(U.cluster, U.probe_table, [{int(a[0]) for a in U.resv_allocs}])
        self.sub = submit_case.random_case(5, 150, U=24, A=8, Q=4, Pn=3)
        self.sub_want = submit_pyref.run(*self.sub)
        run = scen[2].ledger.arrays()[0]
        state = resvq_pyref.NodeState(U.cluster.num_nodes, run, U.resv)
        times = U.now0 + 600 * np.arange(8)
        self.resvq_state = (run, U.resv)
        self.queries = resvq_case.random_queries(3, U.cluster.num_nodes, state, times, 16, lengths=(1, 7, 63, 64, 65))
        self.resvq_want = resvq_pyref.answer(state, int(U.now0), self.queries)
        self.same_resvq = resvq_case.same

    def validate(self, L, i):
        code, elig = L.eng.validate_jobs(self.U.probe_table)
        assert np.array_equal(code, self.valid[0]) and np.array_equal(elig, self.valid[1]), f"cycle {i}: validate_jobs differs from valid_pyref"

    def submit(self, L, i):
        t, jobs, keys = self.sub
        L.eng.set_submit_limits(t)
        code, tlo, adm = L.eng.check_submissions(jobs, keys)
        wcode, wtlo, wadm, wstate = self.sub_want
        assert np.array_equal(code, wcode) and np.array_equal(tlo, wtlo) and adm == wadm, f"cycle {i}: check_submissions differs from submit_pyref"
        got = L.eng.submit_usage()
        assert all(np.array_equal(getattr(got, f), getattr(wstate, f)) for f in wstate.__dataclass_fields__), f"cycle {i}: submit_usage differs from submit_pyref"

    def resvq(self, L, i):
        L.eng.set_resv_query_state(*self.resvq_state)
        self.same_resvq(f"cycle {i}: query_reservations", L.eng.query_reservations(int(self.U.now0), self.queries), self.resvq_want)

    def probe(self, L, i):
        c = self.cycles[i]
        assert L.eng.probe(c.probes).diff(c.probe_expected) is None, f"cycle {i}: a second probe differs from probe_case.expected"

    def download(self, L, i):
        assert L.eng.download().diff(self.cycles[i].oracle.placements) is None, f"cycle {i}: download() differs from the oracle's placements"

    def commit(self, L, i):
        code, counts = L.commit_call(self.cycles[i])
        assert np.array_equal(code, self.cycles[i].code) and np.array_equal(counts, self.cycles[i].counts), f"cycle {i}: a repeated commit_check differs"

    ANYWHERE = ("validate", "submit", "resvq")
    BEHIND_THE_CYCLE = ("probe", "download", "commit")          # cns_probe / cns_download / cns_commit_check: behind step c of the same cycle


@pytest.mark.parametrize("draw", [0, 1])
def test_foreign_calls_anywhere_in_the_loop(engine_default, plain, draw):
    """Six independent calls, each at a seeded random position inside every cycle (those that read the cycle's results: behind step c).
    The loop's own outputs still equal the records, and every foreign answer equals its reference."""
    F = Foreign(plain)
    rng = np.random.default_rng(4000 + draw)
    spots = lc.STEPS + ("end",)
    plan = {}
    for i in range(len(plain[4])):
        for name in F.ANYWHERE:
            plan.setdefault((i, spots[int(rng.integers(0, len(spots)))]), []).append(name)
        for name in F.BEHIND_THE_CYCLE:
            plan.setdefault((i, spots[int(rng.integers(3, len(spots)))]), []).append(name)
    made = []

    def hook(L, i, step):
        for name in plan.get((i, step), ()):
            getattr(F, name)(L, i)
            made.append(name)

    _run(engine_default, plain, hook=hook)
    assert len(made) == 6 * len(plain[4])
    assert len({s for (_, s) in plan}) >= 6, "a condition on the draw: the calls land in front of at least six different steps"


# ---- a refused call in the middle -----------------------------------------------------------------------------------------------------
def _refused(status, words, fn, *a, **kw):
    with pytest.raises(EngineError) as e:
        fn(*a, **kw)
    assert e.value.status == status and words in str(e.value), str(e.value)


@pytest.mark.parametrize("case", ["advance without its mask", "release with an all-zero delta", "order with an account out of range"])
def test_a_refused_call_in_the_middle(engine_default, plain, preempting, case):
    """Cycle 2: one call that is refused for a documented reason (on the host, before any kernel of the call), then the same call made
    correctly.  Every output of that cycle and of the cycles behind it still equals the records."""
    refused = []

    class WithRefusal(Loop):
        def advance_call(self, c, retire, admit):
            if case == "advance without its mask" and c is self.cycles[2]:
                assert self.jobs.num_jobs > 0
                _refused(-1, "missing array: admit", self.eng.advance_running, retire, c.now, np.array(self.queue, np.uint32), None,
                         reservation=self.jobs.reservation, attrs=rap.to_abi(self.U.queue_attrs(self.queue)))
                refused.append(case)
            return super().advance_call(c, retire, admit)

        def release_call(self, rows):
            if case == "release with an all-zero delta" and self.now_cycle == 2 and not refused:
                zero = rows.take(np.arange(rows.num_jobs))
                k = rows.num_jobs // 2
                for f in ("cpu_raw", "mem", "wall_sec", "jobs_count", "submit_count"):
                    getattr(zero, f)[k] = 0
                zero.name_total[k] = 0
                zero.class_count[k] = 0
                _refused(-1, "a delta that is all zero", self.eng.release_usage, zero)
                refused.append(case)
            return super().release_call(rows)

        def order_call(self, c, pd):
            if case == "order with an account out of range" and c is self.cycles[2]:
                bad = self.U.prio_pending(self.survivors)
                bad.account[len(bad.account) // 2] = lc.ACCOUNTS
                _refused(-1, "pending job account >= num_accounts", self.eng.priority_order_resident, c.now, lc.CFG, lc.ACCOUNTS, bad)
                refused.append(case)
            return super().order_call(c, pd)

        def step_g(self, i, c):
            self.now_cycle = i
            super().step_g(i, c)

    if case == "advance without its mask":
        _run(engine_default, preempting, preempt=True, loop=WithRefusal)
    else:
        _run(engine_default, plain, loop=WithRefusal)
    assert refused == [case]
