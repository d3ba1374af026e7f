"""cns_running_amend_ends and cns_resvq_set_state_resident (include/crane_gpu_amend/running_amend.h) on the GPU, in the three-way
pattern of tests/test_gpu_running.py: after every amend the device ledger must equal tests/running_amend_pyref.py's, and the cycle that
follows is run on the engine under test (amended ledger, refilled tables), on a second engine fed cns_set_running(pyref's arrays) and
on the oracle — placements, fp64 cost bit patterns and the time maps of the touched nodes, for equality, no tolerance.  The scenarios
are those of tests/running_amend_case.py; tests/test_running_amend_effect.py holds each of them to the condition that its amendment
changes the next cycle, so a call that skipped the refill fails here."""
import numpy as np
import pytest

from cranesched_amd import abi
from cranesched_amd.engine import EngineError
from tests import resvq_case
from tests import resvq_pyref as rq
from tests import running_amend_case as ac
from tests import running_amend_pyref as ap
from tests import running_pyref as rp
from tests import test_gpu_running as tr
from tests.test_gpu_running import NOW

pytestmark = pytest.mark.gpu
I64_MAX = (1 << 63) - 1


class Trio(tr.Trio):
    def amend(self, led, ids, ends, tag, pairs=None):
        """The amend on the device and on pyref (`led` is changed in place): answers and ledger must agree."""
        found, n = self.eng.amend_running(ids, ends)
        wf, wn = ap.amend(led, ids, ends)
        assert np.array_equal(found, wf) and n == wn, f"{tag}: found {found} / {wf}, written {n} / {wn}"
        self.same_ledger(led, tag)
        if len(ids):
            tm = self.eng.running_amend_timing()
            assert tm["rows"] == len(led.rows), tag
            if pairs is not None:
                assert tm["pairs"] == pairs, f"{tag}: {tm['pairs']} table entries refilled, {pairs} expected"
        return n


def run_case(cls, c: "ac.Case"):
    """Seed, a cycle, the amend, the cycle behind it; the same amendments a second time (the same ends as before), a third cycle."""
    t = Trio(cls, c.cluster, c.resv)
    try:
        led = c.led.copy()
        t.seed(led)
        pairs = t.eng.running_timing()["pairs"]
        if c.entries is not None:
            assert pairs == c.entries
        t.cycle(led, NOW, c.jobs, f"{c.name}: before")
        t.amend(led, c.ids, c.ends, f"{c.name}: amend", pairs=pairs)
        pl = t.cycle(led, NOW, c.jobs, f"{c.name}: after")
        t.amend(led, c.ids, c.ends, f"{c.name}: the same ends again", pairs=pairs)
        t.cycle(led, NOW + 60, c.jobs, f"{c.name}: third cycle")
        return pl
    finally:
        t.close()


# ---- the hand case -------------------------------------------------------------------------------------------------------------
def test_hand_case(engine_default):
    cluster, led, jobs = ac.hand_case()
    t = Trio(engine_default, cluster)
    try:
        t.seed(led)
        pl = t.cycle(led, NOW, jobs, "hand: seeded")
        assert int(pl.start_sec[0]) == NOW + 1000
        for end in (NOW + 500, NOW + 2000):
            assert t.amend(led, [1], [end], f"hand: to {end - NOW}", pairs=1) == 1
            pl = t.cycle(led, NOW, jobs, f"hand: end {end - NOW}")
            assert int(pl.start_sec[0]) == end
        for end in (NOW, I64_MAX, NOW + 1000):   # overdue, never: whatever cns_set_running gives
            t.amend(led, [1], [end], f"hand: to {end}", pairs=1)
            t.cycle(led, NOW, jobs, f"hand: end {end}")
    finally:
        t.close()


# ---- seams ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ac.SIZES)
def test_ledger_size_seams(engine_default, which):
    c = ac.size_case(which)
    if which == "0":
        t = Trio(engine_default, c.cluster)
        try:
            led = c.led.copy()
            t.seed(led)
            assert t.amend(led, [5, 0, ac.U32_MAX], [1, 2, 3], "0 rows: three ids no row carries", pairs=0) == 0
            t.cycle(led, NOW, c.jobs, "0 rows")
        finally:
            t.close()
        return
    run_case(engine_default, c)


@pytest.mark.parametrize("m", ac.ENTRIES)
def test_table_entries_around_the_refills_workgroup(engine_default, m):
    run_case(engine_default, ac.entries_case(m))


@pytest.mark.parametrize("which", ac.KS)
def test_amendment_counts_and_the_ends_of_the_bisection(engine_default, which):
    run_case(engine_default, ac.k_case(which))


def test_ids_no_row_carries_change_nothing(engine_default):
    c = ac.k_case("K=R+3")
    t = Trio(engine_default, c.cluster)
    try:
        led = c.led.copy()
        t.seed(led)
        before = t.eng.running_ledger()
        for ids in ([ac.U32_MAX], [0], [ac.U32_MAX, 77, 0]):
            assert t.amend(led, ids, [NOW + 9] * len(ids), f"misses {ids}") == 0
        assert rp.same_ledger(t.eng.running_ledger(), before) is None
        assert t.amend(led, [], [], "no amendment") == 0
        t.cycle(led, NOW, c.jobs, "misses: the cycle")
    finally:
        t.close()


def test_row_width_seams(engine_default):
    run_case(engine_default, ac.widths_case())


# ---- layouts -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ac.LAYOUTS)
def test_layouts(engine_default, which):
    run_case(engine_default, ac.layout_case(which))


# ---- stale tables --------------------------------------------------------------------------------------------------------------
def test_stale_tables_only_the_ledger_is_written(engine_default):
    c, flipped = ac.stale_case()
    t = Trio(engine_default, c.cluster)
    try:
        led = c.led.copy()
        t.seed(led)
        m = t.eng.running_timing()["pairs"]
        t.amend(led, c.ids[:1], c.ends[-1:], "stale: the normal path first", pairs=m)
        assert m > 0
        t.cluster = flipped
        t.eng.set_nodes(flipped); t.ref.set_nodes(flipped)
        t.amend(led, c.ids, c.ends, "stale: amend behind cns_set_nodes", pairs=0)
        t.advance(led, [], tag="stale: the advance that rebuilds")
        t.cycle(led, NOW, c.jobs, "stale: the cycle")
        # ... which is what a seed of the amended set gives
        fresh = Trio(engine_default, flipped)
        try:
            fresh.seed(led)
            assert fresh.eng.node_select(NOW, c.jobs).diff(t.eng.node_select(NOW, c.jobs)) is None
            assert np.array_equal(fresh.eng.costs().view(np.uint64), t.eng.costs().view(np.uint64))
        finally:
            fresh.close()
    finally:
        t.close()


# ---- composition ---------------------------------------------------------------------------------------------------------------
def test_amend_advance_amend_an_admitted_row(engine_default):
    p = ac.composition_plan()
    t = Trio(engine_default, p.cluster)
    try:
        led = p.led.copy()
        t.seed(led)
        t.amend(led, p.ids, p.ends, "composition: first amend")
        pl = t.cycle(led, p.now, p.jobs, "composition: first cycle")
        nret, nadm = t.advance(led, p.retire, p.now, p.jobs, pl, p.job_ids, tag="composition: boundary")
        assert nret == 2 and nadm >= 3
        ids2, ends2 = p.second(led)
        assert t.amend(led, ids2, ends2, "composition: amend two admitted rows") == 2
        t.cycle(led, p.now + 60, p.jobs2, "composition: second cycle")
    finally:
        t.close()


def test_amend_between_cycles_with_preemption(gpu):
    """The cycle behind the amend equals the one from a fresh seed of the amended set (and cns_set_running + cns_select_preempt, and the
    oracle); the preempt index is refused until that cycle has run."""
    from oracle import pyoracle
    from tests import test_gpu_running_preempt as trp
    from tests.test_preempt import compare_engine, random_preempt_case, run_engine_preempt
    c, j, now, run, pre = random_preempt_case(509, N=10, J=60, P=1, running=14)
    led = rp.Ledger.from_running(run, pre.rn_job_id)
    eng = trp.resident_engine(c, run, pre.rn_job_id)
    fresh = ref = None
    try:
        first = eng.node_select_preempt_resident(now, j, pre)
        eng.preempt_index()
        ids = [int(pre.rn_job_id[-1]), 4242, int(pre.rn_job_id[0]), int(pre.rn_job_id[5])]
        ends = [now + 7000, now + 1, now + 3, now + 7100]
        found, n = eng.amend_running(ids, ends)
        wf, wn = ap.amend(led, ids, ends)
        assert np.array_equal(found, wf) and n == wn == 3
        with pytest.raises(EngineError) as e:
            eng.preempt_index()
        assert e.value.status == -5 and "before a cns_running_select_preempt" in str(e.value)
        run2, _ = led.arrays()
        got = eng.node_select_preempt_resident(now, j, pre)
        fresh = trp.resident_engine(c, run2, pre.rn_job_id)
        trp.same_results("preempt: against a fresh seed", got, fresh.node_select_preempt_resident(now, j, pre))
        ref, rpl, rpo = run_engine_preempt(c, j, now, run2, pre)
        trp.same_results("preempt: against cns_set_running", got, (rpl, rpo))
        ora = pyoracle.select(c, j, now, running=run2, preempt=pre)
        compare_engine("preempt: against the oracle", c, j, ora, eng, *got)
        trp.same_index("preempt: the index built again", eng, led, c, None, now, pre.preempting)
        old = pyoracle.select(c, j, now, running=run, preempt=pre)
        assert (old.placements.diff(ora.placements) is not None or not np.array_equal(old.costs().view(np.uint64), ora.costs().view(np.uint64))), \
            "a condition on the inputs: the amendment changes the cycle with preemption"
        assert first[0].num_jobs == got[0].num_jobs
    finally:
        for e in (eng, fresh, ref):
            if e is not None:
                e.close()


def test_attribute_columns_stay_and_the_consumers_run_on_the_amended_ends(gpu):
    from cranesched_amd.priority import PriorityConfig, PrioPending
    from tests import test_gpu_running_preempt as trp
    from tests import test_gpu_running_preempt_attrs as tpa
    from tests.test_preempt import random_preempt_case
    c, j, now, run, pre = random_preempt_case(509, N=10, J=60, P=1, running=14)
    led = rp.Ledger.from_running(run, pre.rn_job_id)
    a = tpa.attrs_engine(c, run, pre)
    b = None
    try:
        pd = PrioPending(submit_sec=[now - 50, now - 60, now - 70], qos_priority=[1, 2, 3], partition_priority=[1, 1, 2], node_num=[1, 1, 2], total_cpu_raw=[256, 512, 256],
                         total_mem=[1, 2, 3], account=[0, 1, 0])
        cols, order = a.running_attrs(), a.priority_order_resident(now, PriorityConfig(), 2, pd)
        ids = [int(pre.rn_job_id[-1]), int(pre.rn_job_id[0]), int(pre.rn_job_id[5])]
        ends = [now + 7000, now + 3, now + 7100]
        found, n = a.amend_running(ids, ends)
        ap.amend(led, ids, ends)
        assert n == 3 and rp.same_ledger(a.running_ledger(), led.arrays()) is None
        cols2, order2 = a.running_attrs(), a.priority_order_resident(now, PriorityConfig(), 2, pd)
        assert all(cols[f].tobytes() == cols2[f].tobytes() for f in cols), "the columns and the sums, bit for bit"
        assert order[0].tobytes() == order2[0].tobytes() and order[1].tobytes() == order2[1].tobytes() and order[2] == order2[2]
        run2, _ = led.arrays()
        b = trp.resident_engine(c, run2, pre.rn_job_id)
        ra = a.node_select_preempt_resident(now, j, tpa.bare(pre), from_attrs=True)
        rb = b.node_select_preempt_resident(now, j, pre)
        trp.same_results("attrs: from the columns, on the amended ends", ra, rb)
        tpa.same_index("attrs", a, b)
    finally:
        a.close()
        if b is not None:
            b.close()


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_refused_calls_change_nothing(engine_default):
    import ctypes as C
    c = ac.k_case("K=R")
    t = Trio(engine_default, c.cluster)
    try:
        led = c.led.copy()
        t.seed(led)
        want = t.cycle(led, NOW, c.jobs, "refusals: before")
        with pytest.raises(EngineError) as e:
            t.eng.amend_running([9, 17, 9], [1, 2, 3])
        assert e.value.status == -1 and "job id 9 stands twice in job_ids" in str(e.value)
        ids = np.array([9, 17], np.uint32)
        found = np.zeros(2, np.uint8)
        L, h = t.eng._L, t.eng._h
        s = abi.CnsRunningAmend(2, abi._ptr(ids), None)
        o = abi.CnsRunningAmendOut(abi._ptr(found), None)
        assert L.cns_running_amend_ends(h, C.byref(s), C.byref(o)) == -1 and b"missing array: end_sec" in L.cns_last_error(h)
        s = abi.CnsRunningAmend(2, abi._ptr(ids), abi._ptr(np.array([1, 2], np.int64)))
        assert L.cns_running_amend_ends(h, C.byref(s), None) == -1 and b"missing array: out->found" in L.cns_last_error(h)
        t.same_ledger(led, "refusals: the ledger")
        got = t.cycle(led, NOW, c.jobs, "refusals: after")
        assert got.diff(want) is None
    finally:
        t.close()


def test_calls_in_the_wrong_order(gpu):
    from cranesched_amd.engine import GpuNodeSelector
    c = ac.k_case("K=R")
    eng = GpuNodeSelector(device=0)

    def state(fn, *a):
        with pytest.raises(EngineError) as e:
            fn(*a)
        assert e.value.status == -5, str(e.value)
        return str(e.value)

    try:
        assert "before cns_set_nodes" in state(eng.set_resv_query_state_resident, None)
        eng.set_nodes(c.cluster)
        assert "before cns_running_seed" in state(eng.amend_running, [1], [2])
        assert "before cns_running_seed" in state(eng.set_resv_query_state_resident, None)
        run, ids = c.led.arrays()
        eng.seed_running(run, ids)
        eng.amend_running(c.ids, c.ends)
        eng.set_running(run)                                   # drops the ledger
        assert "before cns_running_seed" in state(eng.amend_running, [1], [2])
        eng.seed_running(run, ids)
        eng.set_nodes(tr.flat_cluster(c.cluster.num_nodes + 1))   # another num_nodes drops it too
        assert "before cns_running_seed" in state(eng.amend_running, [1], [2])
        assert "before cns_running_seed" in state(eng.set_resv_query_state_resident, None)
    finally:
        eng.close()


# ---- independence --------------------------------------------------------------------------------------------------------------
def test_other_calls_answer_as_without_an_amend(engine_default):
    """cns_probe, cns_commit_check, cns_usage_apply and the admit step of an advance behind an amend are those of the last cycle."""
    from tests import helpers
    from tests import usage_case as uc
    cluster, jobs, now, run = helpers.random_case(5, N=24, J=80, P=2, running=12)
    ids = 1000 + np.arange(len(run.end_sec))
    probes = helpers.random_case(6, N=24, J=30, P=2, running=0)[1]
    tab, rows = uc.random_case(7, 200, uc.REL)
    answers = []
    for amend in (False, True):
        eng = engine_default(device=0)
        try:
            eng.set_nodes(cluster)
            eng.seed_running(run, ids)
            pl = eng.node_select(now, jobs)
            eng.set_usage_tables(tab)
            if amend:
                assert eng.amend_running([1000, 1005, 7], [now + 9000, now + 1, now])[1] == 2
            p = eng.probe(probes)
            code, counts = eng.commit_check(None, abi.CommitJobs(time_limit_sec=jobs.time_limit_sec))
            nf, of, clean = eng.release_usage(rows)
            assert eng.download().diff(pl) is None
            found, nret, nadm = eng.advance_running([1001], now, 50000 + np.arange(jobs.num_jobs))
            led_run, led_ids = eng.running_ledger()
            answers.append((p, code.copy(), counts.copy(), nf.copy(), of.copy(), clean, nret, nadm, led_ids.copy(), led_run.alloc_node.copy(), led_run.end_sec.copy()))
        finally:
            eng.close()
    a, b = answers
    assert a[0].diff(b[0]) is None and all(np.array_equal(x, y) for x, y in zip(a[1:5], b[1:5])) and a[5:8] == b[5:8]
    assert np.array_equal(a[8], b[8]) and np.array_equal(a[9], b[9])
    changed = np.nonzero(a[10] != b[10])[0]
    assert [int(a[8][x]) for x in changed] == [1000, 1005], "only the two amended rows differ, and they were kept by the advance"


# ---- reservation what-ifs from the ledger ---------------------------------------------------------------------------------------
def _what_if(eng, ref, led, resv, cluster, queries, tag, now=NOW):
    run, ids = led.arrays()
    run = run if len(ids) else None
    eng.set_resv_query_state_resident(resv)
    ref.set_resv_query_state(run, resv)
    want = rq.answer(rq.NodeState(cluster.num_nodes, run, resv), now, queries)
    got = eng.query_reservations(now, queries)
    resvq_case.same(f"{tag} [ledger]", got, want)
    resvq_case.same(f"{tag} [handed in]", ref.query_reservations(now, queries), want)
    return got


def test_reservation_what_ifs_follow_the_amended_ledger(engine_default):
    w = ac.what_if_case()
    eng, ref = engine_default(device=0), engine_default(device=0)
    try:
        for e in (eng, ref):
            e.set_nodes(w.cluster)
        led = w.led.copy()
        eng.seed_running(*led.arrays())
        a0 = _what_if(eng, ref, led, w.resv, w.cluster, w.queries, "what-if: seeded")
        assert a0["code"][:4].tolist() == [rq.FREE, rq.RUNNING, rq.RESERVED, rq.NOT_FOUND] and int(a0["start_sec"][1]) == NOW + 1000
        eng.amend_running(w.ids, w.ends)
        # the tables keep their state until they are set again
        resvq_case.same("what-if: not set again", eng.query_reservations(NOW, w.queries), a0)
        ap.amend(led, w.ids, w.ends)
        a1 = _what_if(eng, ref, led, w.resv, w.cluster, w.queries, "what-if: amended")
        assert a1["code"][:2].tolist() == [rq.RUNNING, rq.FREE] and int(a1["start_sec"][1]) == NOW + 800
        # ... and behind an advance that retires a row; without reservations; from an empty ledger
        eng.advance_running([3])
        led.retire([3])
        _what_if(eng, ref, led, None, w.cluster, w.queries, "what-if: row 3 retired, no reservations")
        eng.advance_running([1, 2])
        led.retire([1, 2])
        a2 = _what_if(eng, ref, led, w.resv, w.cluster, w.queries, "what-if: empty ledger")
        assert a2["code"][:2].tolist() == [rq.FREE, rq.FREE] and int(a2["start_sec"][1]) == NOW
    finally:
        eng.close(); ref.close()


def test_reservation_what_ifs_on_a_random_cluster(engine_default):
    """tests/resvq_case.py's cluster of 300 nodes: the running side through the ledger, rows inside reservations included."""
    cluster, running, resv, times = resvq_case.random_cluster(1, 300)
    state = rq.NodeState(cluster.num_nodes, running, resv)
    queries = resvq_case.random_queries(1, cluster.num_nodes, state, times, 40)
    led = rp.Ledger.from_running(running, 1000 + np.arange(len(running.end_sec)))
    eng, ref = engine_default(device=0), engine_default(device=0)
    try:
        for e in (eng, ref):
            e.set_nodes(cluster)
        eng.seed_running(*led.arrays())
        _what_if(eng, ref, led, resv, cluster, queries, "random: seeded", resvq_case.NOW)
        ids = led.ids()[::3]
        ends = [int(times[i % len(times)]) for i in range(len(ids))]
        eng.amend_running(ids, ends)
        ap.amend(led, ids, ends)
        _what_if(eng, ref, led, resv, cluster, queries, "random: amended", resvq_case.NOW)
    finally:
        eng.close(); ref.close()
