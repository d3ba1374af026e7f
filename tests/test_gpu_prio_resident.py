"""cns_priority_order_resident (include/crane_gpu_running/running_attrs.h) — the MultiFactorPriority sorter with its running side
taken from the device ledger — against three oracles per case:
  1. cns_priority_order on a second engine, fed a PrioRunning assembled on the host from running_ledger() + running_attrs() of the
     engine under test (the columns as downloaded, the per-row sums added up here from the ledger's allocations);
  2. tests/prio_pyref.py: ordered, fed the rows of tests/running_attrs_pyref.py;
  3. for one small case, expected values worked out by hand.
order and num_ordered are compared for equality, the priorities as bit patterns.  The seams come from cns_running_shape."""
import ctypes as C

import numpy as np
import pytest

from cranesched_amd import abi
from cranesched_amd.priority import PriorityConfig, PrioPending, PrioRunning, synth_priority_case
from tests import prio_pyref
from tests import running_attrs_pyref as rap
from tests import running_pyref as rp
from tests.test_gpu_running import NOW, flat_cluster, queue
from tests.test_running_attrs_pyref import CFG as SPREAD_CFG, PENDING as SPREAD_PENDING, spread_rows

pytestmark = pytest.mark.gpu
NODES = 64
GIB = 1 << 30


def alloc(node, cpu=256, mem=GIB):
    return (node, {"cpu_raw": cpu, "mem": mem, "core_lo": 0, "core_hi": 0, "core_w2": 0, "core_w3": 0, "gres": 0})


def ledger(widths, cpus=None, mems=None, first_id=1000):
    """Row i holds widths[i] allocations on consecutive nodes, each of cpus[i] (default: 256 * (1 + i % 4)) and mems[i]."""
    rows = []
    for i, w in enumerate(widths):
        c = cpus[i] if cpus is not None else 256 * (1 + i % 4)
        m = mems[i] if mems is not None else GIB * (1 + i % 3)
        rows.append(rp.Row(first_id + i, NOW + 1000 + i, abi.RESV_NONE, [alloc((5 * i + t) % NODES, c, m) for t in range(int(w))]))
    return rp.Ledger(rows)


def attr_ledger(led, accounts, seed=3, account=None):
    a = rap.random_attrs(np.random.default_rng(seed), len(led.rows), accounts, NOW)
    if account is not None:
        a["account"] = [int(x) for x in account]
    return rap.AttrLedger(led, a)


def pending_dicts(pd):
    return [dict(submit=int(pd.submit_sec[i]), qos=int(pd.qos_priority[i]), part=int(pd.partition_priority[i]), nodes=int(pd.node_num[i]), cpu_raw=int(pd.total_cpu_raw[i]),
                 mem=int(pd.total_mem[i]), account=int(pd.account[i]), cached=float(pd.cached_priority[i]) if pd.cached_priority is not None else 0.0)
            for i in range(pd.num_jobs)]


def cfg_dict(cfg):
    return dict(max_age=cfg.max_age_sec, w_age=cfg.weight_age, w_fair=cfg.weight_fair_share, w_size=cfg.weight_job_size, w_part=cfg.weight_partition, w_qos=cfg.weight_qos,
                favor_small=cfg.favor_small)


def host_running(eng) -> PrioRunning:
    """What a caller without the resident call would hand in: the downloaded columns, and the sums added up here from the ledger."""
    run, _ = eng.running_ledger()
    at = eng.running_attrs()
    off = run.alloc_offsets.astype(np.int64)
    cpu = np.array([int(run.alloc_cpu_raw[off[i]:off[i + 1]].sum()) for i in range(len(off) - 1)], np.int64)
    mem = np.array([int(run.alloc_mem[off[i]:off[i + 1]].sum(dtype=np.uint64)) for i in range(len(off) - 1)], np.uint64)
    return PrioRunning(start_sec=at["start_sec"], qos_priority=at["qos_priority"], partition_priority=at["partition_priority"], node_num=np.diff(off).astype(np.uint32),
                       alloc_cpu_raw=cpu, alloc_mem=mem, account=at["account"])


class Sorter:
    """The engine under test with a ledger that carries columns, a second engine for cns_priority_order, and the Python reference."""

    def __init__(self, cls, ref: rap.AttrLedger, nodes=NODES):
        self.eng, self.host = cls(device=0), cls(device=0)
        self.eng.set_nodes(flat_cluster(nodes))
        self.ref = ref
        run, ids = ref.ledger.arrays()
        self.eng.seed_running(run if len(ids) else None, ids, attrs=rap.to_abi(ref.columns()))

    def check(self, pd, accounts, cfg=None, now=NOW, limit=None, tag=""):
        cfg = cfg or PriorityConfig()
        got = self.eng.priority_order_resident(now, cfg, accounts, pd, limit=limit)
        rn = host_running(self.eng)
        assert rap.same_attrs(self.eng.running_attrs(), self.ref) is None, tag
        want = self.host.priority_order(now, cfg, accounts, pd, running=rn if rn.num_jobs else None, limit=limit)
        assert got[2] == want[2] == min(pd.num_jobs, pd.num_jobs if limit is None else limit), tag
        assert np.array_equal(got[0], want[0]), f"{tag}: the order differs from cns_priority_order's"
        assert np.array_equal(got[1].view(np.uint64), want[1].view(np.uint64)), f"{tag}: the priorities differ from cns_priority_order's in their bits"
        order, prio = prio_pyref.ordered(now, cfg_dict(cfg), pending_dicts(pd), self.ref.pyref_running())
        assert list(got[0]) == order, f"{tag}: the order differs from prio_pyref's"
        assert np.array_equal(got[1].view(np.uint64), np.array(prio, np.float64).view(np.uint64)), f"{tag}: the priorities differ from prio_pyref's in their bits"
        return got

    def close(self):
        self.eng.close()
        self.host.close()


@pytest.fixture(scope="module")
def shape(built):
    from cranesched_amd.engine import lib
    v = [C.c_uint32(0) for _ in range(4)]
    assert lib().cns_running_shape(*[C.byref(x) for x in v]) == 0
    return [x.value for x in v]


def pending(J, accounts, seed=1, cached_frac=0.0):
    return synth_priority_case(J, 0, accounts, seed, now=NOW, cached_frac=cached_frac)[0]


# ---- the hand case ------------------------------------------------------------------------------------------------------------
def test_hand_written_expected_values(engine_default):
    """Two accounts.  Row 0 (account 0): one allocation of 1 cpu / 100 B, started 10 s ago.  Row 1 (account 1): two allocations of 1 cpu /
    100 B each, started 20 s ago: node_num 2, 2 cpus, 200 B.  Pending: job 0 (account 0, 1 cpu, qos 1, 100 s old), job 1 (account 1,
    2 cpus, qos 3, 300 s old), both 1 node / 100 B.  Bounds: cpus 1..2, nodes 1..2, mem 100..200, qos 1..3, age 100..300.  Service
    values: row 0 is at every minimum: 0 * 10 s = 0; row 1 at every maximum: 3 * 20 s = 60; so sv 0..60.
    Job 0: age 0, qos 0, fair 1 - 0 / 60 = 1  ->  100 * 1 = 100.  Job 1: age 1, qos 1, fair 1 - 60 / 60 = 0  ->  1000 + 10 = 1010."""
    led = rp.Ledger([rp.Row(1, NOW + 9, abi.RESV_NONE, [alloc(0, 256, 100)]), rp.Row(2, NOW + 9, abi.RESV_NONE, [alloc(1, 256, 100), alloc(2, 256, 100)])])
    ref = rap.AttrLedger(led, {"start_sec": [NOW - 10, NOW - 20], "qos": [0, 0], "qos_priority": [1, 3], "partition_priority": [1, 1], "account": [0, 1]})
    s = Sorter(engine_default, ref)
    at = s.eng.running_attrs()
    assert list(at["node_num"]) == [1, 2] and list(at["alloc_cpu_raw"]) == [256, 512] and list(at["alloc_mem"]) == [100, 200]
    pd = PrioPending(submit_sec=[NOW - 100, NOW - 300], qos_priority=[1, 3], partition_priority=[1, 1], node_num=[1, 1], total_cpu_raw=[256, 512], total_mem=[100, 100], account=[0, 1])
    cfg = PriorityConfig(max_age_sec=1000, weight_age=1000, weight_fair_share=100, weight_job_size=0, weight_partition=0, weight_qos=10, favor_small=True)
    order, prio, n = s.check(pd, 2, cfg, tag="hand")
    assert list(order) == [1, 0] and list(prio) == [100.0, 1010.0] and n == 2
    s.close()


# ---- sizes ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["0", "1", "chunk-1", "chunk+1"])
def test_ledger_sizes(engine_default, shape, which):
    """R of 0, 1 and job_chunk -+ 1; rows of 1, 2 and lane_max_allocs + 1 allocations."""
    job_chunk, lane_max = shape[0], shape[1]
    R = {"chunk-1": job_chunk - 1, "chunk+1": job_chunk + 1}.get(which) or int(which)
    s = Sorter(engine_default, attr_ledger(ledger([(1, 2, lane_max + 1)[i % 3] for i in range(R)]), 5))
    s.check(pending(300, 5), 5, tag=which)
    s.close()


@pytest.mark.parametrize("accounts", [1, 255, 256, 257, 65537])
def test_account_counts(engine_default, accounts):
    """The key sort's pass counts: 0 (one account), 1, 1, 2 and 3 passes; the largest id is in use on both sides."""
    R = 40
    acc = np.random.default_rng(accounts).integers(0, accounts, R)
    acc[7] = accounts - 1
    acc[11] = 0
    s = Sorter(engine_default, attr_ledger(ledger([1 + i % 3 for i in range(R)]), accounts, account=acc))
    pd = pending(200, accounts)
    pd.account[5] = accounts - 1
    s.check(pd, accounts, tag=f"A = {accounts}")
    s.close()


def test_rows_per_account(engine_default, shape):
    """An account without a running row, with 7, 8 and 9 rows (the unrolled sum's seam), and — after a retire — one with all rows."""
    lane_max = shape[1]
    acc = [1] * 7 + [2] * 8 + [3] * 9
    acc = [acc[(5 * i) % 24] for i in range(24)]      # interleaved: an account's rows are not neighbours
    s = Sorter(engine_default, attr_ledger(ledger([(1, lane_max + 1)[i % 2] for i in range(24)]), 4, account=acc))
    pd = pending(150, 4)
    s.check(pd, 4, tag="0 / 7 / 8 / 9 rows")
    gone = [r.job_id for r, a in zip(s.ref.ledger.rows, s.ref.rows) if a["account"] != 3]
    s.eng.advance_running(gone, attrs=True)
    s.ref.retire(gone)
    assert len(s.ref.rows) == 9
    s.check(pd, 4, tag="every row in one account")
    s.close()


def test_all_bounds_equal(engine_default):
    """Every job, pending or running, with the same cpus, nodes, memory, QoS and partition priority and the same age: the `else`
    branches of the service terms (each adds 1.0) and no factor but fair share."""
    R, J = 12, 40
    led = ledger([1] * R, cpus=[512] * R, mems=[GIB] * R)
    ref = rap.AttrLedger(led, {"start_sec": [NOW - 100 - 7 * i for i in range(R)], "qos": [0] * R, "qos_priority": [10] * R, "partition_priority": [5] * R,
                               "account": [i % 3 for i in range(R)]})
    pd = PrioPending(submit_sec=[NOW - 500] * J, qos_priority=[10] * J, partition_priority=[5] * J, node_num=[1] * J, total_cpu_raw=[512] * J, total_mem=[GIB] * J,
                     account=[i % 4 for i in range(J)])
    s = Sorter(engine_default, ref)
    _, prio, _ = s.check(pd, 4, tag="all bounds equal")
    assert len(set(prio)) == 4, "four accounts, four fair-share values"
    s.close()


def test_cached_priorities_a_limit_and_the_same_call_twice(engine_default, shape):
    s = Sorter(engine_default, attr_ledger(ledger([1 + i % 4 for i in range(60)]), 9))
    pd = pending(500, 9, cached_frac=0.3)
    assert (pd.cached_priority != 0).any() and (pd.cached_priority == 0).any()
    a = s.check(pd, 9, tag="cached")
    b = s.check(pd, 9, tag="cached, again")
    assert np.array_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes()
    c = s.check(pd, 9, limit=123, tag="limit")
    assert c[2] == 123 and np.array_equal(a[0], c[0])
    t = s.eng.priority_timing()
    assert t["kernels_ms"] > 0 and t["algorithmic_bytes"] > 500 * 300
    s.close()


def test_the_order_of_the_rows_decides_the_last_bits(engine_default):
    """tests/test_running_attrs_pyref.py: spread_rows — an account whose rows' service terms span more than twenty binades.  Summed in
    ledger order and in the reverse order its fp64 value differs, and with fair share as the only weight that difference is the last
    bit of a priority (checked here on the CPU first — otherwise the case shows nothing about order).  The device gives the
    ledger-order one."""
    ref = spread_rows()
    cfg = PriorityConfig(weight_age=0, weight_fair_share=1, weight_job_size=0, weight_partition=0, weight_qos=0)
    assert cfg_dict(cfg) == SPREAD_CFG
    pd = PrioPending(**{k: [j[v] for j in SPREAD_PENDING] for k, v in (("submit_sec", "submit"), ("qos_priority", "qos"), ("partition_priority", "part"), ("node_num", "nodes"),
                                                                      ("total_cpu_raw", "cpu_raw"), ("total_mem", "mem"), ("account", "account"))})
    fwd = prio_pyref.ordered(NOW, SPREAD_CFG, pending_dicts(pd), ref.pyref_running())[1]
    rev = prio_pyref.ordered(NOW, SPREAD_CFG, pending_dicts(pd), ref.pyref_running()[::-1])[1]
    assert fwd[1] != rev[1], "a condition on the inputs: the reversed order shows in a priority"
    s = Sorter(engine_default, ref, nodes=8)
    _, prio, _ = s.check(pd, 3, cfg, tag="spread")
    assert prio[1] == fwd[1] != rev[1]
    s.close()


def test_the_call_after_each_of_four_advances(engine_default):
    """Cycles with jobs ending and starting: the sorter reads what each boundary left on the device."""
    rng = np.random.default_rng(8)
    s = Sorter(engine_default, attr_ledger(ledger([1 + i % 3 for i in range(30)]), 6))
    pd = pending(400, 6)
    for c in range(4):
        now = NOW + 60 * c
        jobs = queue([1, 2, 1, 3, 1, 1, 2, 1])
        pl = s.eng.node_select(now, jobs)
        ids = s.ref.ledger.ids()
        retire = ids[c::5]
        job_ids = 50000 + 100 * c + np.arange(jobs.num_jobs)
        qa = rap.random_attrs(rng, jobs.num_jobs, 6, now, start=False)
        _, nret, nadm = s.eng.advance_running(retire, now, job_ids, attrs=rap.to_abi(qa))
        s.ref.retire(retire)
        assert nadm == s.ref.admit(pl, jobs.time_limit_sec, now, job_ids, qa) > 0 and nret == len(retire) > 0
        s.check(pd, 6, now=now + 30, tag=f"after advance {c}")
    s.close()


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def _raw_call(eng, pd, accounts):
    """The C call with sentinel-filled outputs -> (status, message, outputs)."""
    J = pd.num_jobs
    order, prio, n = np.full(J, 0xABABABAB, np.uint32), np.full(J, -7.25), C.c_uint64(0xFEED)
    c_cfg, c_pd = PriorityConfig().to_c(), pd.to_c()
    rc = eng._L.cns_priority_order_resident(eng._h, C.c_int64(NOW), C.byref(c_cfg), C.c_uint32(accounts), C.byref(c_pd), C.c_uint64(J), order.ctypes.data_as(C.c_void_p),
                                            prio.ctypes.data_as(C.c_void_p), C.byref(n))
    return rc, eng._L.cns_last_error(eng._h).decode(), (order, prio, n.value)


def _untouched(out):
    order, prio, n = out
    return (order == 0xABABABAB).all() and (prio == -7.25).all() and n == 0xFEED


@pytest.mark.parametrize("case", ["account", "cpu past int64", "memory past uint64", "negative cpu"])
def test_a_bad_row_is_refused_by_the_device_and_the_next_valid_call_is_exact(engine_default, shape, case):
    lane_max = shape[1]
    R, A = 300, 5
    widths = [1 + i % 3 for i in range(R)]
    cpus, mems, acc = [256] * R, [GIB] * R, [i % A for i in range(R)]
    bad = [257, 40, 123]                       # the least of three offending rows decides; one sits in the second workgroup
    if case == "account":
        for r in bad:
            acc[r] = A
        status, words = -1, "ledger row 40 carries account 5, num_accounts is 5"
    elif case == "cpu past int64":
        for r in bad:
            widths[r], cpus[r] = 2, 1 << 62    # 2^63
        widths[40] = lane_max + 1              # ... and the wave's sum: (lane_max + 1) * 2^62
        status, words = -4, "ledger row 40 sum to a cpu value outside int64"
    elif case == "memory past uint64":
        for r in bad:
            widths[r], mems[r] = 2, 1 << 63    # 2^64
        status, words = -4, "ledger row 40 sum to a cpu value outside int64 or a memory value outside uint64"
    else:
        for r in bad:
            widths[r], cpus[r] = 3, -1
        status, words = -1, "ledger row 40's allocations sums to a negative value"
    ref = attr_ledger(ledger(widths, cpus, mems), A, account=acc)
    assert ref.first_bad_row(A) == (40, {"account": "account", "cpu past int64": "range", "memory past uint64": "range", "negative cpu": "negative"}[case])
    s = Sorter(engine_default, ref)
    pd = pending(100, A)
    for _ in range(2):                         # (the second call meets the sums the first one left)
        rc, msg, out = _raw_call(s.eng, pd, A)
        assert rc == status and words in msg, msg
        assert _untouched(out), "nothing is written to the outputs on a refusal"
    gone = [ref.ledger.rows[r].job_id for r in bad]
    s.eng.advance_running(gone, attrs=True)
    s.ref.retire(gone)
    assert s.ref.first_bad_row(A) is None
    s.check(pd, A, tag=f"{case}: the next valid call")
    s.close()


def test_no_ledger_and_no_columns(engine_default):
    from cranesched_amd.engine import EngineError
    eng = engine_default(device=0)
    eng.set_nodes(flat_cluster(NODES))
    pd = pending(10, 3)
    rc, msg, out = _raw_call(eng, pd, 3)
    assert rc == -5 and "before cns_running_seed_attrs" in msg and _untouched(out)
    run, ids = ledger([1, 2, 1]).arrays()
    eng.seed_running(run, ids)
    rc, msg, out = _raw_call(eng, pd, 3)
    assert rc == -5 and "carries no attribute columns" in msg and _untouched(out)
    with pytest.raises(EngineError):
        eng.running_attrs()
    eng.seed_running(run, ids, attrs=abi.RunningAttrs(qos=[0, 0, 0], qos_priority=[1, 2, 3], partition_priority=[1, 1, 1], account=[0, 1, 2], start_sec=[NOW - 5] * 3))
    assert eng.priority_order_resident(NOW, PriorityConfig(), 3, pd)[2] == 10
    eng.close()
