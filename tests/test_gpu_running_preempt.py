"""A cycle with preemption on the device-resident running set (include/crane_gpu_running/running_preempt.h).  Truth in every case is
twofold: a second engine fed the same ledger through cns_set_running + cns_select_preempt, and the oracle (for the three-cycle run also
tests/running_pyref.py for the ledger).  Placements, reasons, start times, preempted lists in push-back order, cancelled ids in call
order and the preempting set must be equal, without a tolerance, and the index the device built (preempt_index()) must equal
tests/running_preempt_pyref.py after every call.  The seams come from cns_running_shape."""
import numpy as np
import pytest

from cranesched_amd import abi
from oracle import pyoracle
from tests import kat_preempt
from tests import running_preempt_pyref as rpp
from tests import running_pyref as rp
from tests.test_gpu_running import GIB, NOW, flat_cluster
from tests.test_preempt import compare_engine, overlap_preempt_case, random_preempt_case, resv_preempt_case, run_engine_preempt

pytestmark = pytest.mark.gpu


def same_results(tag, a, b):
    """(placements, PreemptOut) of the engine under test against the second engine's."""
    (pl, po), (rpl, rpo) = a, b
    d = pl.diff(rpl)
    assert d is None, f"{tag}: placements differ from cns_set_running + cns_select_preempt: {d}"
    assert po.lists() == rpo.lists(), f"{tag}: preempted lists {po.lists()} vs {rpo.lists()}"
    assert po.cancelled_ids() == rpo.cancelled_ids(), f"{tag}: cancelled {po.cancelled_ids()} vs {rpo.cancelled_ids()}"
    assert po.preempting_ids() == rpo.preempting_ids(), f"{tag}: preempting set {po.preempting_ids()} vs {rpo.preempting_ids()}"


def same_as_oracle(tag, c, j, ora, eng, pl, po, resv):
    if resv is None:
        return compare_engine(tag, c, j, ora, eng, pl, po)
    d = pl.diff(ora.placements)   # (with reservations every node has a time map: tests/test_preempt.py, test_engine_preempt_with_reservations)
    assert d is None, f"{tag}: engine placements differ from the oracle: {d}"
    assert po.lists() == ora.preempt_out.lists() and po.cancelled_ids() == ora.preempt_out.cancelled_ids() and po.preempting_ids() == ora.preempt_out.preempting_ids(), tag
    assert np.array_equal(eng.costs().view(np.uint64), ora.costs().view(np.uint64)), f"{tag}: fp64 costs differ"
    for n in range(c.num_nodes):
        a, b = eng.timeline(n), ora.timeline(n)
        for f in ("t", "cpu_raw", "mem", "core_lo", "core_hi", "gres"):
            assert np.array_equal(a[f], b[f]), f"{tag}: time map of node {n}, field {f}"


def same_index(tag, eng, led, c, resv, now, preempting):
    f = rpp.same_index(eng.preempt_index(), rpp.index(led, *rpp.layout_of(c, resv), now, [int(x) for x in preempting]))
    assert f is None, f"{tag}: the device-built index differs from running_preempt_pyref in {f}"


def resident_engine(c, run, ids, resv=None, **cfg):
    from cranesched_amd.engine import GpuNodeSelector
    eng = GpuNodeSelector(device=0, **cfg)
    eng.set_nodes(c)
    if resv is not None:
        eng.set_reservations(resv)
    eng.seed_running(run if run is not None and len(run.end_sec) else None, ids)
    return eng


def check_case(tag, c, j, now, run, pre, resv=None, oracle=True):
    """One cycle on the engine under test, the second engine and the oracle; -> (engine under test, its results, second engine)."""
    eng = resident_engine(c, run, pre.rn_job_id, resv)
    ref, rpl, rpo = run_engine_preempt(c, j, now, run, pre, resv=resv)
    try:
        pl, po = eng.node_select_preempt_resident(now, j, pre)
        same_results(tag, (pl, po), (rpl, rpo))
        assert eng.last_kernel().split(" [")[0] == ref.last_kernel().split(" [")[0], f"{tag}: {eng.last_kernel()} vs {ref.last_kernel()}"   # (without a split cycle's timing note)
        if oracle:
            ora = pyoracle.select(c, j, now, running=run, reservations=resv, preempt=pre)
            same_as_oracle(tag, c, j, ora, eng, pl, po, resv)
        same_index(tag, eng, rp.Ledger.from_running(run, pre.rn_job_id), c, resv, now, pre.preempting)
    except BaseException:
        eng.close(); ref.close()
        raise
    return eng, (pl, po), ref


# ---- 1. known answers ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scn", kat_preempt.scenarios(), ids=lambda s: s[0])
def test_known_answers(gpu, scn):
    name, c, j, r, pre, expect = scn
    eng, (pl, po), ref = check_case(name, c, j, kat_preempt.NOW, r, pre)
    try:
        has_list = any(len(pre.qos_preempt[int(q)]) for q in pre.pd_qos)
        assert eng.last_kernel().startswith("k_select") == has_list
        assert po.cancelled_ids() == expect["cancelled"] and po.preempting_ids() == expect["preempting"]
    finally:
        eng.close(); ref.close()


# ---- 2. random cases -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(12))
def test_random_cases(gpu, seed):
    c, j, now, run, pre = random_preempt_case(500 + seed, N=6 + seed % 7, J=50 + seed % 40, P=1 + seed % 2, running=10 + seed % 11)
    eng, _, ref = check_case(f"random {seed}", c, j, now, run, pre)
    eng.close(); ref.close()


def test_the_random_cases_preempt(gpu):
    """A condition on the generator: the cases above reach TryPreempt_'s releases."""
    tot = 0
    for seed in range(12):
        c, j, now, run, pre = random_preempt_case(500 + seed, N=6 + seed % 7, J=50 + seed % 40, P=1 + seed % 2, running=10 + seed % 11)
        tot += sum(len(x) for x in pyoracle.select(c, j, now, running=run, preempt=pre).preempt_out.lists())
    assert tot > 10, tot


@pytest.mark.parametrize("seed", range(4))
def test_rows_inside_reservations(gpu, seed):
    c, j, now, run, rv, pre = resv_preempt_case(seed)
    assert run.reservation is not None and (run.reservation != abi.RESV_NONE).any(), "a condition on the inputs: rows on virtual slots"
    eng, _, ref = check_case(f"resv {seed}", c, j, now, run, pre, resv=rv)
    eng.close(); ref.close()


@pytest.mark.parametrize("seed,lay", [(0, "all+subsets"), (1, "chain"), (2, "random"), (3, "all+subsets")])
def test_partitions_that_share_nodes(gpu, seed, lay):
    c, j, now, run, pre = overlap_preempt_case(seed, layout=lay)
    eng, _, ref = check_case(f"overlap {seed} {lay}", c, j, now, run, pre)
    try:
        x = eng.preempt_index()
        assert len(x["ent_job"]) > len(run.alloc_node), "a condition on the inputs: one allocation is several entries"
    finally:
        eng.close(); ref.close()


# ---- 3. seams ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shape(built):
    from cranesched_amd.engine import lib
    import ctypes as C
    v = [C.c_uint32(0) for _ in range(4)]
    assert lib().cns_running_shape(*[C.byref(x) for x in v]) == 0
    return [x.value for x in v]   # job_chunk, lane_max_allocs, sort_tile, scan_span


def _alloc(node, core):
    return (node, {"cpu_raw": 256, "mem": GIB, "core_lo": (1 << core) if core < 64 else 0, "core_hi": (1 << (core - 64)) if core >= 64 else 0,
                   "core_w2": 0, "core_w3": 0, "gres": 0})


def ledger_of(n, widths, skip=()):
    """Row i holds widths[i] allocations of one core each on consecutive nodes (never on a node of `skip`), core k for the k-th
    allocation on a node; ids 1000 + i; ends spread behind NOW."""
    ok = [x for x in range(n) if x not in skip]
    per_node, rows, at = {}, [], 0
    for i, w in enumerate(widths):
        al = []
        for _ in range(int(w)):
            node = ok[at % len(ok)]; at += 1
            k = per_node.get(node, 0); per_node[node] = k + 1
            assert k < 100
            al.append(_alloc(node, k))
        rows.append(rp.Row(1000 + i, NOW + 100 + 13 * (i % 50), abi.RESV_NONE, al))
    return rp.Ledger(rows)


def tiny_queue(cpus=128, n_jobs=4):
    """A handful of one-node jobs of `cpus` cores each (the nodes have 128)."""
    one = np.ones(n_jobs, np.uint32)
    return abi.Jobs(partition=np.zeros(n_jobs, np.uint32), time_limit_sec=600 + 60 * np.arange(n_jobs, dtype=np.int64), node_mem=np.zeros(n_jobs, np.uint64),
                    task_cpu_raw=np.full(n_jobs, cpus * 256, np.int64), task_mem=np.full(n_jobs, GIB, np.uint64), node_num=one, ntasks=one,
                    ntasks_per_node_min=one, ntasks_per_node_max=one)


def tiny_preempt(led, jobs, preempting=()):
    """One preempting QoS: every pending job (QoS 1) may preempt every running job (QoS 0); distinct start times and priorities."""
    R, J = len(led.rows), jobs.num_jobs
    return abi.Preempt([[], [0]], 1 + np.arange(J), np.ones(J, np.uint32), np.full(J, 20, np.uint32), J - np.arange(J, dtype=np.float64) + 0.5,
                       np.array(led.ids(), np.uint32), np.zeros(R, np.uint32), np.full(R, 10, np.uint32), NOW - 1 - 7 * np.arange(R, dtype=np.int64),
                       preempting=list(preempting))


def check_ledger(tag, n, led, sched=None, preempting=None, expect_preemptions=True):
    c = flat_cluster(n, sched=sched)
    ids = led.ids()
    # every job asks for one core more than the emptiest schedulable node has free: it starts there by preempting one running job
    held = [sum(1 for r in led.rows for a in r.allocs if a[0] == x) for x in range(n) if sched is None or sched[x]]
    jobs = tiny_queue(128 - min(held) + 1 if ids else 128)
    pre = tiny_preempt(led, jobs, preempting if preempting is not None else ([ids[0], ids[-1], 4242] if ids else [4242]))
    run, _ = led.arrays()
    eng, (pl, po), ref = check_case(tag, c, jobs, NOW, run if ids else None, pre)
    try:
        if expect_preemptions:
            assert sum(len(x) for x in po.lists()) > 0, f"{tag}: a condition on the inputs: the queue preempts"
        return eng.preempt_index()
    finally:
        eng.close(); ref.close()


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_ledger_rows_around_a_workgroup(gpu, shape, delta):
    R = shape[0] + delta
    check_ledger(f"{R} rows", 5, ledger_of(5, [1] * R))


def test_rows_of_lane_max_allocations_and_one_more(gpu, shape):
    lane_max = shape[1]
    x = check_ledger("wide rows", 24, ledger_of(24, [1, lane_max, lane_max + 1, 2, lane_max + 1, lane_max, 1]))
    assert sorted(np.diff(x["rj_off"]).tolist()) == sorted([1, lane_max, lane_max + 1, 2, lane_max + 1, lane_max, 1])


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_pair_count_around_a_sort_tile(gpu, shape, delta):
    m = shape[2] + delta
    x = check_ledger(f"{m} pairs", 300, ledger_of(300, [1] * m))
    assert len(x["ent_job"]) == m


@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_a_row_without_any_entry(gpu, where):
    """Node 3 is not schedulable: a row whose only allocation is there has no entry; it stands first, in the middle, last."""
    n, R = 8, 9
    led = ledger_of(n, [2] * R, skip=(3,))
    at = {"first": 0, "middle": R // 2, "last": R - 1}[where]
    led.rows[at].allocs = [_alloc(3, 0)]
    sched = np.ones(n, np.uint8); sched[3] = 0
    x = check_ledger(f"no entry {where}", n, led, sched=sched, preempting=[led.ids()[at], led.ids()[(at + 1) % R]])
    assert x["rj_off"][at] == x["rj_off"][at + 1] and x["rj_end"][at] == 0 and x["rj_preempting"][at] == 1


def test_a_ledger_of_zero_rows(gpu):
    x = check_ledger("zero rows", 8, rp.Ledger([]), expect_preemptions=False)
    assert x["rj_off"].tolist() == [0] and len(x["ent_job"]) == 0


# ---- 4. the preempting set -----------------------------------------------------------------------------------------------------
def _case4():
    c, j, now, run, pre = random_preempt_case(509, N=10, J=60, P=1, running=14)
    return c, j, now, run, pre


def _with_set(pre, ids):
    return abi.Preempt(pre.qos_preempt, pre.pd_job_id, pre.pd_qos, pre.pd_qos_priority, pre.pd_priority, pre.rn_job_id, pre.rn_qos, pre.rn_qos_priority,
                       pre.rn_start_sec, preempting=list(ids))


@pytest.mark.parametrize("which", ["empty", "every row", "an unknown id", "an id twice"])
def test_the_preempting_set(gpu, which):
    c, j, now, run, pre = _case4()
    ids = [int(x) for x in pre.rn_job_id]
    pre = _with_set(pre, {"empty": [], "every row": ids[::-1], "an unknown id": [4242], "an id twice": [ids[3], ids[5], ids[3]]}[which])
    eng, (pl, po), ref = check_case(which, c, j, now, run, pre)
    try:
        x = eng.preempt_index()
        want = {"empty": 0, "every row": len(ids), "an unknown id": 0, "an id twice": 2}[which]
        assert int(x["rj_preempting"].sum()) == want
        assert set(pre.preempting.tolist()) & set(ids) <= set(po.preempting_ids()) and 4242 not in po.preempting_ids()
        # the resident end times are as before the call: a plain cycle behind it is the second engine's plain cycle, and the oracle's
        plain = pyoracle.select(c, j, now, running=run)
        for e in (eng, ref):
            assert e.node_select(now, j).diff(plain.placements) is None, f"{which}: the patched end times leaked into the next plain cycle"
    finally:
        eng.close(); ref.close()


def test_the_set_of_one_call_is_passed_to_the_next(gpu):
    c, j, now, run, pre = _case4()
    eng, (pl, po), ref = check_case("call c", c, j, now, run, pre)
    try:
        assert po.cancelled_ids(), "a condition on the inputs: call c preempts running jobs"
        pre2 = _with_set(pre, po.preempting_ids())
        pl2, po2 = eng.node_select_preempt_resident(now + 5, j, pre2)
        same_results("call c + 1", (pl2, po2), ref.node_select_preempt(now + 5, j, pre2))
        ora = pyoracle.select(c, j, now + 5, running=run, preempt=pre2)
        compare_engine("call c + 1", c, j, ora, eng, pl2, po2)
        same_index("call c + 1", eng, rp.Ledger.from_running(run, pre.rn_job_id), c, None, now + 5, pre2.preempting)
        assert set(po.preempting_ids()) <= set(po2.preempting_ids())
    finally:
        eng.close(); ref.close()


# ---- 5. enabled without lists --------------------------------------------------------------------------------------------------
def test_enabled_without_lists_runs_the_fast_kernels(gpu):
    c, j, now, run, pre = random_preempt_case(555, N=12, J=120, P=2, running=18)
    pre = abi.Preempt([[], [], []], pre.pd_job_id, pre.pd_qos, pre.pd_qos_priority, pre.pd_priority, pre.rn_job_id, pre.rn_qos, pre.rn_qos_priority,
                      pre.rn_start_sec, preempting=[1001, 1003, 4242])
    eng, (pl, po), ref = check_case("no lists", c, j, now, run, pre)
    try:
        assert not eng.last_kernel().startswith("k_select"), eng.last_kernel()
        assert po.lists() == [[] for _ in range(j.num_jobs)] and po.cancelled_ids() == [] and po.preempting_ids() == [1001, 1003]
        # ... which is cns_select with the marked rows ending at now + 1
        end = run.end_sec.copy(); end[[1, 3]] = now + 1
        marked = abi.Running(end, run.alloc_offsets, run.alloc_node, run.alloc_cpu_raw, run.alloc_mem, run.alloc_core_lo, run.alloc_core_hi, run.alloc_gres)
        ref.set_running(marked)
        assert pl.diff(ref.node_select(now, j)) is None
    finally:
        eng.close(); ref.close()


# ---- 6. three consecutive cycles -----------------------------------------------------------------------------------------------
def test_three_consecutive_cycles(engine_cls):
    """Cycle c through the new call, then cns_running_advance with retire_ids = the cancelled ids of cycle c and admit = the jobs with
    reason none that start now and preempted no running job (the commit loop holds the others back).  After every advance the ledger
    equals running_pyref's; cycle c + 1 equals the second engine fed cns_set_running from cns_running_get, and the oracle."""
    c, j, now, run, pre = random_preempt_case(503, N=10, J=60, P=2, running=14)
    J = j.num_jobs
    led = rp.Ledger.from_running(run, pre.rn_job_id)
    info = {int(i): (int(q), int(p), int(s)) for i, q, p, s in zip(pre.rn_job_id, pre.rn_qos, pre.rn_qos_priority, pre.rn_start_sec)}
    eng, ref = engine_cls(device=0), engine_cls(device=0)
    try:
        for e in (eng, ref):
            e.set_nodes(c)
        eng.seed_running(*led.arrays())
        preempting, preempted_any = list(pre.preempting), 0
        for cyc in range(3):
            t = now + 60 * cyc
            ids = led.ids()
            p = abi.Preempt(pre.qos_preempt, pre.pd_job_id, pre.pd_qos, pre.pd_qos_priority, pre.pd_priority, np.array(ids, np.uint32),
                            [info[i][0] for i in ids], [info[i][1] for i in ids], [info[i][2] for i in ids], preempting=preempting)
            got_run, got_ids = eng.running_ledger()
            assert rp.same_ledger((got_run, got_ids), led.arrays()) is None, f"cycle {cyc}: the device ledger differs from running_pyref"
            ref.set_running(got_run if len(got_ids) else None)
            pl, po = eng.node_select_preempt_resident(t, j, p)
            same_results(f"cycle {cyc}", (pl, po), ref.node_select_preempt(t, j, p))
            ora = pyoracle.select(c, j, t, running=led.arrays()[0], preempt=p)
            compare_engine(f"cycle {cyc}", c, j, ora, eng, pl, po)
            same_index(f"cycle {cyc}", eng, led, c, None, t, preempting)
            lists = po.lists()
            preempted_any += sum(len(x) for x in lists)
            admit = np.array([int(pl.reason[x]) == 0 and int(pl.start_sec[x]) == t and not any(not pending for pending, _ in lists[x]) for x in range(J)], np.uint8)
            job_ids = 50000 + 1000 * cyc + np.arange(J)
            retire = po.cancelled_ids()
            found, nret, nadm = eng.advance_running(retire, t, job_ids, admit)
            wf, wr = led.retire(retire)
            wa = led.admit(pl, j.time_limit_sec, t, job_ids, admit)
            assert np.array_equal(found, wf) and (nret, nadm) == (wr, wa), f"boundary {cyc}"
            assert rp.same_ledger(eng.running_ledger(), led.arrays()) is None, f"boundary {cyc}: the device ledger differs from running_pyref"
            for x in np.nonzero(admit)[0]:
                info[int(job_ids[x])] = (int(pre.pd_qos[x]), int(pre.pd_qos_priority[x]), now - 7 * (100 + 100 * cyc + int(x)) - 3)   # (a start no other row has: nothing is left unordered)
            preempting = po.preempting_ids()
        assert preempted_any > 0, "a condition on the inputs: the cycles preempt"
    finally:
        eng.close(); ref.close()


# ---- 7. refusals on the device -------------------------------------------------------------------------------------------------
def _raises(status, fn, *a, **kw):
    from cranesched_amd.engine import EngineError
    with pytest.raises(EngineError) as e:
        fn(*a, **kw)
    assert e.value.status == status, str(e.value)
    return str(e.value)


@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_an_rn_job_id_that_is_not_the_ledgers(gpu, where):
    c, j, now, run, pre = _case4()
    eng = resident_engine(c, run, pre.rn_job_id)
    try:
        before = eng.node_select(now, j)
        R = len(pre.rn_job_id)
        row = {"first": 0, "middle": R // 2, "last": R - 1}[where]
        ids = pre.rn_job_id.copy(); ids[row] = 77777
        if where == "first":
            ids[R - 1] = 88888   # the least row that differs is named
        bad = abi.Preempt(pre.qos_preempt, pre.pd_job_id, pre.pd_qos, pre.pd_qos_priority, pre.pd_priority, ids, pre.rn_qos, pre.rn_qos_priority, pre.rn_start_sec,
                          preempting=pre.preempting)
        msg = _raises(-1, eng.node_select_preempt_resident, now, j, bad)
        assert f"rn_job_id[{row}] is 77777, ledger row {row} carries job id {int(pre.rn_job_id[row])}" in msg, msg
        # no cycle has run: the results of the cycle before stand, and so does the admit step's right to them
        assert eng.download().diff(before) is None
        eng.advance_running([], now, 50000 + np.arange(j.num_jobs))
    finally:
        eng.close()


def test_calls_in_the_wrong_order(gpu):
    from cranesched_amd.engine import GpuNodeSelector
    c, j, now, run, pre = _case4()
    eng = GpuNodeSelector(device=0)
    try:
        assert "before cns_set_nodes" in _raises(-5, eng.node_select_preempt_resident, now, j, pre)
        eng.set_nodes(c)
        assert "before cns_running_seed" in _raises(-5, eng.node_select_preempt_resident, now, j, pre)
        assert "before a cns_running_select_preempt" in _raises(-5, eng.preempt_index)
        eng.seed_running(run, pre.rn_job_id)
        assert "before a cns_running_select_preempt" in _raises(-5, eng.preempt_index)
        eng.set_running(run)                                  # drops the ledger
        assert "before cns_running_seed" in _raises(-5, eng.node_select_preempt_resident, now, j, pre)
        eng.seed_running(run, pre.rn_job_id)
        eng.set_nodes(c)                                      # empties the per-slot tables, the ledger survives
        assert "are not the ledger's" in _raises(-5, eng.node_select_preempt_resident, now, j, pre)
        eng.advance_running([])
        assert "cns_set_running" in _raises(-5, eng.node_select_preempt, now, j, pre)   # cns_select_preempt keeps refusing device-built tables
        pl, po = eng.node_select_preempt_resident(now, j, pre)
        assert "missing array: admit" in _raises(-1, eng.advance_running, [], now, 50000 + np.arange(j.num_jobs))
        eng.advance_running([], now, 50000 + np.arange(j.num_jobs), np.zeros(j.num_jobs, np.uint8))
        assert "before a cns_running_select_preempt" in _raises(-5, eng.preempt_index)   # the index described the tables before the advance
    finally:
        eng.close()


# ---- 8. neighbours unchanged ---------------------------------------------------------------------------------------------------
def test_other_calls_answer_as_behind_cns_select_preempt(gpu):
    from tests import helpers
    from tests import usage_case as uc
    c, j, now, run, pre = _case4()
    eng, (pl, po), ref = check_case("neighbours", c, j, now, run, pre)
    try:
        probes = helpers.random_case(6, N=c.num_nodes, J=10, P=1, running=0)[1]
        for e in (eng, ref):
            assert "after a cycle with preemption" in _raises(-4, e.probe, probes)
        tab, rows = uc.random_case(7, 200, uc.REL)
        ans = []
        for e in (eng, ref):
            e.set_usage_tables(tab)
            code, counts = e.commit_check(None, abi.CommitJobs(time_limit_sec=j.time_limit_sec))
            nf, of, clean = e.release_usage(rows)
            ans.append((code.copy(), counts.copy(), nf.copy(), of.copy(), clean))
        assert all(np.array_equal(x, y) for x, y in zip(ans[0][:4], ans[1][:4])) and ans[0][4] == ans[1][4]
        # ... and a plain cycle behind it is served by cns_probe again
        eng.node_select(now, j)
        eng.probe(probes)
    finally:
        eng.close(); ref.close()
