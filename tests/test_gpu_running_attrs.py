"""The attribute columns beside the device ledger (include/crane_gpu_running/running_attrs.h) against tests/running_attrs_pyref.py.
After every call running_attrs() of the engine under test must equal the Python reference — the five columns and the three per-row
sums — and its running_ledger() must equal what a second engine gives that made the same calls without attributes (and pyref's
ledger).  Equality everywhere.  The seams come from cns_running_shape; the small inputs are those of tests/test_gpu_running.py."""
import numpy as np
import pytest

from cranesched_amd import abi
from cranesched_amd.priority import PriorityConfig, PrioPending
from tests import helpers
from tests import running_attrs_pyref as rap
from tests import running_case as rc
from tests import running_pyref as rp
from tests.test_gpu_running import NOW, flat_cluster, queue, running

pytestmark = pytest.mark.gpu
ACCOUNTS = 5


class Pair:
    """The engine under test (ledger with columns), a second engine that makes the plain calls, and the Python reference."""

    def __init__(self, cls, cluster, led: rp.Ledger, seed=1):
        self.rng = np.random.default_rng(seed)
        self.eng, self.plain = cls(device=0), cls(device=0)
        self.eng.set_nodes(cluster)
        self.plain.set_nodes(cluster)
        self.ref = rap.AttrLedger(led, rap.random_attrs(self.rng, len(led.rows), ACCOUNTS, NOW))
        run, ids = led.arrays()
        self.eng.seed_running(run if len(ids) else None, ids, attrs=rap.to_abi(self.ref.columns()))
        self.plain.seed_running(run if len(ids) else None, ids)
        self.same("seed")

    def same(self, tag):
        f = rap.same_attrs(self.eng.running_attrs(), self.ref)
        assert f is None, f"{tag}: running_attrs() differs from the reference in {f}"
        got = self.eng.running_ledger()
        f = rp.same_ledger(got, self.plain.running_ledger()) or rp.same_ledger(got, self.ref.ledger.arrays())
        assert f is None, f"{tag}: the ledger differs in {f}"

    def cycle(self, now, jobs):
        pl = self.eng.node_select(now, jobs)
        assert self.plain.node_select(now, jobs).diff(pl) is None
        return pl

    def advance(self, retire, now=None, jobs=None, pl=None, job_ids=None, admit=None, tag=""):
        if job_ids is None:
            got = self.eng.advance_running(retire, attrs=True)
            want = self.plain.advance_running(retire)
            wf, wr = self.ref.retire(retire)
            wa = 0
        else:
            qa = rap.random_attrs(self.rng, jobs.num_jobs, ACCOUNTS, now, start=False)
            qa["start_sec"] = [7] * jobs.num_jobs   # handed in and not read
            got = self.eng.advance_running(retire, now, job_ids, admit, attrs=rap.to_abi(qa))
            want = self.plain.advance_running(retire, now, job_ids, admit)
            wf, wr = self.ref.retire(retire)
            wa = self.ref.admit(pl, jobs.time_limit_sec, now, job_ids, qa, admit)
        assert np.array_equal(got[0], want[0]) and got[1:] == want[1:], f"{tag}: the answers differ from the plain call's"
        assert np.array_equal(got[0], wf) and got[1:] == (wr, wa), f"{tag}: the answers differ from the reference's"
        self.same(tag)
        return got[1], got[2]

    def close(self):
        self.eng.close()
        self.plain.close()


@pytest.fixture(scope="module")
def shape(built):
    import ctypes as C
    from cranesched_amd.engine import lib
    v = [C.c_uint32(0) for _ in range(4)]
    assert lib().cns_running_shape(*[C.byref(x) for x in v]) == 0
    return [x.value for x in v]


@pytest.fixture(scope="module")
def scen(built):
    return rc.scenario(11)


def test_four_consecutive_cycles(engine_default, scen):
    """tests/running_case.py: every boundary retires and admits, the columns follow."""
    cluster, first, cycles = scen
    p = Pair(engine_default, cluster, first.copy())
    for i, c in enumerate(cycles):
        pl = p.cycle(c.now, c.jobs)
        assert pl.diff(c.oracle.placements) is None
        nret, nadm = p.advance(c.retire, c.now, c.jobs, c.oracle.placements, c.job_ids, admit=c.admit, tag=f"boundary {i}")
        assert (nret, nadm) == (c.num_retired, c.num_admitted) and nadm >= 10 and nret >= 1
        assert rp.same_ledger(p.ref.ledger.arrays(), c.after.arrays()) is None
        assert list(p.ref.columns()["start_sec"][-nadm:]) == [c.now] * nadm
    p.close()


@pytest.mark.parametrize("which", ["0", "1", "chunk-1", "chunk", "chunk+1"])
def test_ledger_size_seams(engine_default, shape, which):
    """Ledgers of 0, 1 and job_chunk - 1 / = / + 1 rows: seed; a boundary that retires the first, a middle and the last row and admits
    every job of a cycle; one that does nothing; one that retires every row."""
    job_chunk = shape[0]
    R = {"chunk-1": job_chunk - 1, "chunk": job_chunk, "chunk+1": job_chunk + 1}.get(which) or int(which)
    n = 300
    p = Pair(engine_default, flat_cluster(n), running(n, [1] * R))
    jobs = queue([1, 2, 1, 3, 1, 1, 2, 1])
    pl = p.cycle(NOW, jobs)
    ids = p.ref.ledger.ids()
    retire = sorted({ids[0], ids[-1], ids[len(ids) // 2]}) if ids else []
    nret, nadm = p.advance(retire + [77], NOW, jobs, pl, 50000 + np.arange(jobs.num_jobs), tag=f"{which}: retire three, admit all")
    assert nret == len(retire) and nadm == jobs.num_jobs
    assert p.advance([], tag=f"{which}: retire none, admit none") == (0, 0)
    everything = p.ref.ledger.ids()
    assert p.advance(everything[::-1], tag=f"{which}: retire all") == (len(everything), 0)
    assert len(p.eng.running_attrs()["account"]) == 0
    p.close()


def test_allocations_per_job_seams(engine_default, shape):
    """Rows of 1, lane_max_allocs, lane_max_allocs + 1, 64 and 65 allocations, seeded and admitted: a lane sums its row, or the row is
    handed to the wave, in one and in two steps."""
    lane_max = shape[1]
    widths = [1, lane_max, lane_max + 1, 64, 65]
    n = 160
    p = Pair(engine_default, flat_cluster(n), running(n, [2] + widths + widths[::-1] + [3], stride=11))
    assert sorted(set(p.eng.running_attrs()["node_num"])) == sorted(set(widths + [2, 3]))
    jobs = queue(widths + [1] + widths[::-1])
    pl = p.cycle(NOW, jobs)
    assert ((pl.reason[:jobs.num_jobs] == 0) & (pl.start_sec[:jobs.num_jobs] == NOW)).all(), "a condition on the inputs: every width is admitted"
    p.advance([p.ref.ledger.ids()[0], p.ref.ledger.ids()[6]], NOW, jobs, pl, 50000 + np.arange(jobs.num_jobs), tag="widths: boundary")
    got = p.eng.running_attrs()
    assert list(got["node_num"][-len(jobs.node_num):]) == list(jobs.node_num) and list(got["alloc_cpu_raw"][-3:]) == [256 * w for w in widths[::-1][-3:]]
    p.advance([50003, 50004], tag="widths: retire two admitted wide rows")
    p.close()


@pytest.mark.parametrize("case", ["retire first", "retire last", "retire all, admit all", "admit none of a queue", "one row"])
def test_retire_and_admit(engine_default, case):
    cluster, jobs, now, run = helpers.random_case(21, N=24, J=120, P=2, running=1 if case == "one row" else 20)
    p = Pair(engine_default, cluster, rp.Ledger.from_running(run, 1000 + np.arange(len(run.end_sec))))
    pl = p.cycle(now, jobs)
    J = jobs.num_jobs
    started = (pl.reason[:J] == 0) & (pl.start_sec[:J] == now)
    assert started.any() and not started.all()
    ids, job_ids = p.ref.ledger.ids(), 50000 + np.arange(J)
    if case in ("retire first", "retire last"):
        assert p.advance([ids[0] if case == "retire first" else ids[-1]], tag=case) == (1, 0)
    elif case == "retire all, admit all":
        assert p.advance(ids, now, jobs, pl, job_ids, tag=case) == (len(ids), int(started.sum()))
        assert p.ref.ledger.ids() == list(job_ids[started])
    elif case == "admit none of a queue":
        assert p.advance([], now, jobs, pl, job_ids, admit=np.zeros(J, np.uint8), tag=case) == (0, 0)
    else:
        assert len(ids) == 1
        assert p.advance([], now, jobs, pl, job_ids, tag=case + ": admit") == (0, int(started.sum()))
        assert p.advance(ids, tag=case + ": retire the seeded row") == (1, 0)
    p.close()


def test_a_refused_advance_leaves_the_columns_and_a_plain_advance_drops_them(engine_default):
    """The time map's cap, provoked as tests/test_gpu_running.py provokes it: the 1007th allocation on one node, by admit, is
    CNS_ERR_UNSUPPORTED and leaves ledger and columns bit for bit.  A plain advance_running behind it drops the columns: running_attrs()
    and the two consumers return CNS_ERR_STATE and say why."""
    from cranesched_amd.engine import EngineError
    tiny = {"cpu_raw": 1, "mem": 1, "core_lo": 0, "core_hi": 0, "core_w2": 0, "core_w3": 0, "gres": 0}
    led = rp.Ledger([rp.Row(1000 + i, NOW + 1000, abi.RESV_NONE, [(0, dict(tiny))]) for i in range(1006)])
    p = Pair(engine_default, flat_cluster(4), led)
    jobs = queue([1, 1], incl=[[0], [1]])
    pl = p.cycle(NOW, jobs)
    assert list(pl.reason[:2]) == [0, 0] and list(pl.node_idx[:2]) == [0, 1]
    before = p.eng.running_attrs()
    qa = rap.to_abi(rap.random_attrs(p.rng, 2, ACCOUNTS, NOW, start=False))
    with pytest.raises(EngineError) as e:
        p.eng.advance_running([3], NOW, 50000 + np.arange(2), attrs=qa)
    assert e.value.status == -4 and "too many running allocations" in str(e.value)
    after = p.eng.running_attrs()
    assert all(before[f].tobytes() == after[f].tobytes() for f in before), "the columns and the sums, bit for bit"
    p.same("after the refusal")
    # ... the call without its admit step is served, and so is the sorter on what it leaves
    p.advance([1003], tag="retire one")
    pd = PrioPending(submit_sec=[NOW - 50, NOW - 60], qos_priority=[1, 2], partition_priority=[1, 1], node_num=[1, 1], total_cpu_raw=[256, 512], total_mem=[1, 2], account=[0, 1])
    p.eng.priority_order_resident(NOW, PriorityConfig(), ACCOUNTS, pd)
    # ... a plain advance drops the columns
    p.eng.advance_running([])
    pre = abi.Preempt(qos_preempt=[[]], pd_job_id=[1, 2], pd_qos=[0, 0], pd_qos_priority=[0, 0], pd_priority=[0.0, 0.0], rn_job_id=[], rn_qos=[], rn_qos_priority=[], rn_start_sec=[])
    for call in (p.eng.running_attrs, lambda: p.eng.priority_order_resident(NOW, PriorityConfig(), ACCOUNTS, pd),
                 lambda: p.eng.node_select_preempt_resident(NOW, jobs, pre, from_attrs=True), lambda: p.eng.advance_running([], attrs=True)):
        with pytest.raises(EngineError) as e:
            call()
        assert e.value.status == -5 and "carries no attribute columns" in str(e.value), str(e.value)
    assert rp.same_ledger(p.eng.running_ledger(), p.ref.ledger.arrays()) is None, "the ledger itself stays"
    p.close()
