"""The running set kept on the device (include/crane_gpu_running/running.h) against tests/running_pyref.py and the existing yardsticks.
After every call the device ledger must equal pyref's; the cycle that follows is run on the engine under test, on a second engine fed
by cns_set_running(pyref's arrays) and on the oracle, and all three must agree bit for bit: placements, fp64 costs (they fail on any
slip in per-slot order) and the time maps of every touched node.  Equality everywhere, no tolerance.  The seams come from
cns_running_shape."""
import numpy as np
import pytest

from cranesched_amd import abi
from oracle import pyoracle
from tests import helpers
from tests import running_case as rc
from tests import running_pyref as rp

pytestmark = pytest.mark.gpu
NOW = 1_700_000_000
GIB = 1 << 30
FULL = np.uint64(0xFFFFFFFFFFFFFFFF)


# ---- small deterministic inputs ----------------------------------------------------------------------------------------------
def flat_cluster(n, parts=None, sched=None):
    """n nodes of 128 cores; parts: node lists per partition (default: one partition over all)."""
    parts = parts if parts is not None else [np.arange(n)]
    off = np.cumsum([0] + [len(p) for p in parts]).astype(np.uint32)
    return abi.Cluster(np.full(n, 128 * 256, np.int64), np.full(n, 512 * GIB, np.uint64), np.full(n, FULL), np.full(n, FULL), np.zeros(n, np.uint64),
                       off, np.concatenate(parts).astype(np.uint32), schedulable=sched)


def queue(widths, partition=0, incl=None, resv=None, limit=None):
    """One job per entry of widths: that many nodes, one task of one cpu on each."""
    k = np.asarray(widths, np.uint32)
    j = len(k)
    kw = {}
    if incl is not None:   # per job a node list (or None)
        off, flat = [0], []
        for lst in incl:
            flat += list(lst or [])
            off.append(len(flat))
        kw = dict(incl_offsets=np.array(off, np.uint64), incl_nodes=np.array(flat or [0], np.uint32))
    return abi.Jobs(partition=np.broadcast_to(np.asarray(partition, np.uint32), (j,)).copy(), time_limit_sec=np.asarray(limit if limit is not None else 600 + 60 * np.arange(j), np.int64),
                    node_mem=np.zeros(j, np.uint64), task_cpu_raw=np.full(j, 256, np.int64), task_mem=np.full(j, GIB, np.uint64), node_num=k, ntasks=k,
                    ntasks_per_node_min=np.ones(j, np.uint32), ntasks_per_node_max=np.ones(j, np.uint32), reservation=resv, **kw)


def running(n, widths, resv=None, first_id=1000, end=None, stride=7):
    """Job i holds widths[i] allocations of one core each on consecutive nodes from (i * stride) % n; the k-th allocation on a node takes
    core k (at most 128 per node).  -> rp.Ledger"""
    per_node = np.zeros(n, np.int64)
    rows = []
    for i, w in enumerate(widths):
        al = []
        for t in range(int(w)):
            node = (i * stride + t) % n
            c = int(per_node[node]); per_node[node] += 1
            assert c < 128
            al.append((node, {"cpu_raw": 256, "mem": GIB, "core_lo": (1 << c) if c < 64 else 0, "core_hi": (1 << (c - 64)) if c >= 64 else 0,
                              "core_w2": 0, "core_w3": 0, "gres": 0}))
        rows.append(rp.Row(first_id + i, int(end[i]) if end is not None else NOW + 100 + 13 * (i % 50), int(resv[i]) if resv is not None else abi.RESV_NONE, al))
    return rp.Ledger(rows)


class Trio:
    """The engine under test (device ledger), a second engine fed by cns_set_running, and the oracle, on one cluster."""

    def __init__(self, cls, cluster, resv=None, **cfg):
        self.cluster, self.resv, self.cfg = cluster, resv, cfg
        self.eng, self.ref = cls(device=0, **cfg), cls(device=0, **cfg)
        for e in (self.eng, self.ref):
            e.set_nodes(cluster)
            if resv is not None:
                e.set_reservations(resv)

    def set_reservations(self, resv):
        self.resv = resv
        self.eng.set_reservations(resv)
        self.ref.set_reservations(resv)

    def seed(self, led):
        run, ids = led.arrays()
        self.eng.seed_running(run if len(ids) else None, ids)
        self.same_ledger(led, "seed")

    def same_ledger(self, led, tag):
        f = rp.same_ledger(self.eng.running_ledger(), led.arrays())
        assert f is None, f"{tag}: the device ledger differs from pyref in {f}"

    def cycle(self, led, now, jobs, tag):
        """One cycle on all three from the ledger `led`; -> the placements (they are the same)."""
        run, ids = led.arrays()
        run = run if len(ids) else None
        self.ref.set_running(run)
        ora = pyoracle.select(self.cluster, jobs, now, running=run, reservations=self.resv, **self.cfg)
        touched = rc.touched_nodes(self.cluster, led, placements=ora.placements)[:48]
        in_part = np.zeros(self.cluster.num_nodes, bool)
        in_part[np.asarray(self.cluster.part_nodes, np.int64)] = True
        want_tl = {n: ora.timeline(n) for n in touched if in_part[n]}
        got = None
        for name, e in (("device ledger", self.eng), ("cns_set_running", self.ref)):
            pl = e.node_select(now, jobs)
            helpers.assert_same(e, pl, ora, self.cluster, sample_nodes=8, tag=f"{tag} [{name}]")
            for n, w in want_tl.items():
                g = e.timeline(n)
                for f in w:
                    assert np.array_equal(g[f], w[f]), f"{tag} [{name}]: time map of node {n} differs in {f}"
            got = got or pl
        return got

    def advance(self, led, retire, now=None, jobs=None, placements=None, job_ids=None, admit=None, tag=""):
        """The boundary on the device and on pyref (`led` is changed in place); answers and ledger must agree."""
        resv = jobs.reservation if jobs is not None else None
        found, nret, nadm = self.eng.advance_running(retire, now, job_ids, admit, resv if job_ids is not None else None)
        wf, wr = led.retire(retire)
        wa = led.admit(placements, jobs.time_limit_sec, now, job_ids, admit, resv) if job_ids is not None else 0
        assert np.array_equal(found, wf) and (nret, nadm) == (wr, wa), f"{tag}: found {found} / {wf}, retired {nret} / {wr}, admitted {nadm} / {wa}"
        self.same_ledger(led, tag)
        return nret, nadm

    def close(self):
        self.eng.close()
        self.ref.close()


@pytest.fixture(scope="module")
def shape(built):
    from cranesched_amd.engine import lib
    import ctypes as C
    v = [C.c_uint32(0) for _ in range(4)]
    assert lib().cns_running_shape(*[C.byref(x) for x in v]) == 0
    job_chunk, lane_max, sort_tile, scan_span = [x.value for x in v]
    return job_chunk, lane_max, sort_tile, scan_span


def _ledger_sizes():
    return ["0", "1", "63", "64", "65", "chunk-1", "chunk", "chunk+1", "scan carry"]


# ---- seams ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", _ledger_sizes())
def test_ledger_size_seams(engine_default, shape, which):
    """Ledger sizes around a wave, a workgroup and the row scan's carry (64 * scan_span + 1 rows are one per-wave count more than a
    step of the scan takes), on about 300 nodes: more than 256 slots, a second digit pass of the sort.  Seed, a cycle, a boundary that
    retires the first, the last and a middle row and admits the cycle's jobs, the next cycle."""
    job_chunk, _, _, scan_span = shape
    R = {"chunk-1": job_chunk - 1, "chunk": job_chunk, "chunk+1": job_chunk + 1, "scan carry": 64 * scan_span + 1}.get(which) or int(which) if which != "0" else 0
    n = 300
    t = Trio(engine_default, flat_cluster(n))
    led = running(n, [1] * R)
    t.seed(led)
    jobs = queue([1, 2, 1, 3, 1, 1, 2, 1])
    pl = t.cycle(led, NOW, jobs, f"{which}: first cycle")
    ids = led.ids()
    retire = sorted({ids[0], ids[-1], ids[len(ids) // 2]}) if ids else []
    nret, nadm = t.advance(led, retire + [77], NOW, jobs, pl, 50000 + np.arange(jobs.num_jobs), tag=f"{which}: boundary")
    assert nret == len(retire) and nadm == jobs.num_jobs
    t.cycle(led, NOW + 60, queue([1, 1, 4, 1]), f"{which}: second cycle")
    tm = t.eng.running_timing()
    assert tm["jobs"] == len(led.rows) and tm["allocs"] == tm["pairs"] == sum(len(r.allocs) for r in led.rows)
    t.close()


def test_allocations_per_job_seams(engine_default, shape):
    """Rows of 1, lane_max, lane_max + 1, 64 and 65 allocations: copied by their lane, or handed to the wave, in one and in two steps —
    in the ledger (retire compacts them) and in the queue (admit appends them)."""
    _, lane_max, _, _ = shape
    widths = [1, lane_max, lane_max + 1, 64, 65]
    n = 160
    t = Trio(engine_default, flat_cluster(n))
    led = running(n, [2] + widths + widths[::-1] + [3], stride=11)
    t.seed(led)
    jobs = queue(widths + [1] + widths[::-1])
    pl = t.cycle(led, NOW, jobs, "widths: first cycle")
    started = (pl.reason[:jobs.num_jobs] == 0) & (pl.start_sec[:jobs.num_jobs] == NOW)
    assert started.all(), "a condition on the inputs: every width is admitted"
    t.advance(led, [led.ids()[0], led.ids()[6]], NOW, jobs, pl, 50000 + np.arange(jobs.num_jobs), tag="widths: boundary")
    assert sorted(set(len(r.allocs) for r in led.rows)) == sorted(set(widths + [3]))
    t.cycle(led, NOW + 60, queue([1, 2, 1]), "widths: second cycle")
    t.advance(led, [50003, 50004], tag="widths: retire two admitted wide rows")
    t.cycle(led, NOW + 120, queue([1, 2, 1]), "widths: third cycle")
    t.close()


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_pair_count_seams(engine_default, shape, delta):
    """sort_tile - 1 / sort_tile / sort_tile + 1 (slot, allocation) pairs: one tile of the sort, and one element into the second."""
    _, _, sort_tile, _ = shape
    m = sort_tile + delta
    n = 300
    t = Trio(engine_default, flat_cluster(n))
    led = running(n, [1] * m)
    t.seed(led)
    assert t.eng.running_timing()["pairs"] == m
    t.cycle(led, NOW, queue([1, 2, 1]), f"{m} pairs")
    t.close()


# ---- layouts -------------------------------------------------------------------------------------------------------------------
def _shared_cluster(n=40):
    nodes = np.arange(n)
    sched = np.ones(n, np.uint8)
    sched[5] = 0
    return flat_cluster(n, [nodes, nodes[nodes % 2 == 0], nodes[nodes % 3 == 0]], sched)


def _resv(nodes, start, end):
    m = len(nodes)
    return abi.Reservations([start], [end], [0, m], nodes, np.full(m, 64 * 256, np.int64), np.full(m, 256 * GIB, np.uint64), np.full(m, FULL),
                            np.zeros(m, np.uint64), np.zeros(m, np.uint64))


def test_shared_partitions_and_an_unschedulable_node(engine_default):
    """Three partitions over the same nodes: an allocation counts on 1, 2 or 3 slots.  Node 5 is not schedulable: its entry is dropped
    from the per-slot tables and the ledger keeps it."""
    n = 40
    t = Trio(engine_default, _shared_cluster(n))
    led = running(n, [1, 2, 3, 1, 9, 1, 1, 2] * 6, stride=3)
    assert any(a[0] == 5 for r in led.rows for a in r.allocs)
    t.seed(led)
    pairs = sum(1 + (a[0] % 2 == 0) + (a[0] % 3 == 0) for r in led.rows for a in r.allocs if a[0] != 5)
    assert t.eng.running_timing()["pairs"] == pairs
    jobs = queue([1, 2, 1, 3, 1, 1, 2, 1, 1], partition=[0, 1, 2, 0, 1, 2, 0, 1, 2])
    pl = t.cycle(led, NOW, jobs, "shared: first cycle")
    t.advance(led, led.ids()[::5], NOW, jobs, pl, 50000 + np.arange(jobs.num_jobs), tag="shared: boundary")
    t.cycle(led, NOW + 60, jobs, "shared: second cycle")
    t.close()


def test_reservations(engine_default):
    """An active reservation over nodes 2, 3, 4: a running job inside it lands on the virtual slot; one with an unknown reservation index
    and one inside the reservation on a node it does not list land nowhere.  Queue jobs submitted to the reservation are admitted with
    it.  Then cns_set_reservations between two cycles (the running tables are emptied, the ledger survives) and an empty advance."""
    n = 24
    rv = _resv([2, 3, 4], NOW - 100, NOW + 50000)
    t = Trio(engine_default, flat_cluster(n, [np.arange(n), np.arange(0, n, 2)]), rv)
    resv = [abi.RESV_NONE, 0, 0, 5, abi.RESV_NONE, 0]
    rows = []
    for i, (node, r) in enumerate(zip([2, 2, 3, 6, 3, 7], resv)):
        rows.append(rp.Row(900 + i, NOW + 500 + i, r, [(node, {"cpu_raw": 256, "mem": GIB, "core_lo": (1 << i) if r == 0 else 0, "core_hi": 0 if r == 0 else (1 << i), "core_w2": 0, "core_w3": 0,
                                                            "gres": 0})]))   # (the reserved share is the low 64 cores)
    led = rp.Ledger(rows)
    t.seed(led)
    assert t.eng.running_timing()["pairs"] == 2 + 1 + 1 + 0 + 1 + 0      # node 2 has two slots; nodes 2, 3 one virtual slot each
    jobs = queue([1, 1, 2, 1, 1], partition=[0, 1, 0, 0, 1], resv=np.array([abi.RESV_NONE, 0, 0, abi.RESV_NONE, 9], np.uint32))
    pl = t.cycle(led, NOW, jobs, "resv: first cycle")
    assert pl.reason[1] == 0 and pl.reason[2] == 0 and pl.reason[4] == 6, "jobs inside the reservation start; an unknown one is refused"
    t.advance(led, [900], NOW, jobs, pl, 50000 + np.arange(5), tag="resv: boundary")
    assert [r.reservation for r in led.rows if r.job_id in (50001, 50002)] == [0, 0]
    t.cycle(led, NOW + 60, jobs, "resv: second cycle")
    # another reservation table: the virtual slots move, the ledger stays
    t.set_reservations(_resv([3, 7], NOW - 100, NOW + 50000))
    t.same_ledger(led, "resv: after cns_set_reservations")
    t.advance(led, [], tag="resv: empty advance")
    t.cycle(led, NOW + 120, queue([1, 1, 1], partition=[0, 1, 0]), "resv: third cycle")
    t.set_reservations(None)
    t.advance(led, [], tag="resv: empty advance without reservations")
    t.cycle(led, NOW + 180, queue([1, 1, 1], partition=[0, 1, 0]), "resv: fourth cycle")
    t.close()


# ---- retire / admit ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["none", "all", "first", "last", "unknown", "retired and admitted", "mask"])
def test_retire_and_admit(engine_default, case):
    """A queue on a small busy cluster, so that it holds started, backfilled and failed jobs: only the started ones enter."""
    cluster, jobs, now, run = helpers.random_case(21, N=24, J=120, P=2, running=20)
    t = Trio(engine_default, cluster)
    led = rp.Ledger.from_running(run, 1000 + np.arange(len(run.end_sec)))
    t.seed(led)
    pl = t.cycle(led, now, jobs, f"{case}: first cycle")
    J = jobs.num_jobs
    started = (pl.reason[:J] == 0) & (pl.start_sec[:J] == now)
    assert started.any() and ((pl.reason[:J] != 0) & (pl.start_sec[:J] > now)).any() and ((pl.reason[:J] != 0) & (pl.start_sec[:J] == 0)).any()
    ids, job_ids = led.ids(), 50000 + np.arange(J)
    if case == "none":
        nret, nadm = t.advance(led, [], tag=case)
        assert (nret, nadm) == (0, 0) and led.ids() == ids
    elif case == "all":
        nret, nadm = t.advance(led, ids[::-1], now, jobs, pl, job_ids, tag=case)
        assert nret == len(ids) and nadm == int(started.sum()) and led.ids() == list(job_ids[started])
    elif case in ("first", "last"):
        nret, _ = t.advance(led, [ids[0] if case == "first" else ids[-1]], tag=case)
        assert nret == 1 and led.ids() == (ids[1:] if case == "first" else ids[:-1])
    elif case == "unknown":
        before = led.copy()
        found, nret, _ = t.eng.advance_running([4, ids[3], 5])
        assert list(found) == [0, 1, 0] and nret == 1
        led.retire([ids[3]])
        t.same_ledger(led, case)
        assert len(before.rows) == len(led.rows) + 1
    elif case == "retired and admitted":      # retire runs first: the id leaves the ledger and comes back at its end
        job_ids = job_ids.copy()
        job_ids[np.nonzero(started)[0][0]] = ids[2]
        t.advance(led, [ids[2]], now, jobs, pl, job_ids, tag=case)
        assert led.ids().count(ids[2]) == 1 and led.ids().index(ids[2]) == len(ids) - 1
    else:                                     # admit NULL against a mask
        mask = np.zeros(J, np.uint8)
        mask[np.nonzero(started)[0][::2]] = 1
        mask[~started] = 1                    # set on jobs that did not start: they stay out all the same
        other = led.copy()
        t.advance(led, [], now, jobs, pl, job_ids, admit=mask, tag=case)
        other.admit(pl, jobs.time_limit_sec, now, job_ids)
        assert len(led.rows) - len(ids) == int(mask[started].sum()) < len(other.rows) - len(ids) == int(started.sum())
    t.cycle(led, now + 60, jobs, f"{case}: second cycle")
    t.close()


# ---- the cap -------------------------------------------------------------------------------------------------------------------
def test_the_time_map_cap(engine_default):
    """1006 allocations on one node are served; the 1007th, by admit, is CNS_ERR_UNSUPPORTED and leaves the ledger and the running tables
    exactly as they were.  (The allocations end together: the node's time map stays short and the node takes another job.)"""
    from cranesched_amd.engine import EngineError
    n = 4
    t = Trio(engine_default, flat_cluster(n))
    tiny = {"cpu_raw": 1, "mem": 1, "core_lo": 0, "core_hi": 0, "core_w2": 0, "core_w3": 0, "gres": 0}
    led = rp.Ledger([rp.Row(1000 + i, NOW + 1000, abi.RESV_NONE, [(0, dict(tiny))]) for i in range(1006)])
    t.seed(led)
    jobs = queue([1, 1], incl=[[0], [1]])
    pl = t.cycle(led, NOW, jobs, "cap: 1006 on node 0")
    assert list(pl.reason[:2]) == [0, 0] and list(pl.node_idx[:2]) == [0, 1] and list(pl.start_sec[:2]) == [NOW, NOW]
    with pytest.raises(EngineError) as e:
        t.eng.advance_running([3], NOW, 50000 + np.arange(2))
    assert e.value.status == -4 and "too many running allocations" in str(e.value)
    t.same_ledger(led, "cap: after the refusal")
    t.cycle(led, NOW, jobs, "cap: the cycle after the refusal")
    # ... and with room made by the same call's retire the job enters
    t.advance(led, [1000 + 1, 1000 + 2], NOW, jobs, pl, 50000 + np.arange(2), tag="cap: retire two, admit two")
    assert sum(1 for r in led.rows for a in r.allocs if a[0] == 0) == 1005
    with pytest.raises(EngineError) as e:
        t.eng.seed_running(*rp.Ledger(led.rows + [rp.Row(7, NOW + 5, abi.RESV_NONE, [(0, dict(tiny))]), rp.Row(8, NOW + 5, abi.RESV_NONE, [(0, dict(tiny))])]).arrays())
    assert e.value.status == -4
    t.same_ledger(led, "cap: after the refused seed")
    t.cycle(led, NOW + 60, jobs, "cap: last cycle")
    t.close()


# ---- several cycles ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scen(built):
    return rc.scenario(11)


def test_four_consecutive_cycles(engine_cls, scen):
    """tests/running_case.py once per selection kernel: every cycle runs on what the previous boundary left on the device."""
    cluster, first, cycles = scen
    t = Trio(engine_cls, cluster)
    t.seed(first)
    for i, c in enumerate(cycles):
        t.same_ledger(c.before, f"cycle {i}: before")
        pl = t.cycle(c.before, c.now, c.jobs, f"cycle {i}")
        assert pl.diff(c.oracle.placements) is None
        led = c.before.copy()
        nret, nadm = t.advance(led, c.retire, c.now, c.jobs, pl, c.job_ids, admit=c.admit, tag=f"boundary {i}")
        assert (nret, nadm) == (c.num_retired, c.num_admitted) and nadm >= 10 and nret >= 1
        t.same_ledger(c.after, f"cycle {i}: after")
    t.close()


# ---- independence --------------------------------------------------------------------------------------------------------------
def test_other_calls_answer_as_without_an_advance(engine_default):
    """cns_probe, cns_commit_check and cns_usage_apply before and after an advance give the same answers."""
    from tests import usage_case as uc
    cluster, jobs, now, run = helpers.random_case(5, N=24, J=80, P=2, running=12)
    eng = engine_default(device=0)
    eng.set_nodes(cluster)
    eng.seed_running(run, 1000 + np.arange(len(run.end_sec)))
    eng.node_select(now, jobs)
    probes = helpers.random_case(6, N=24, J=30, P=2, running=0)[1]
    tab, rows = uc.random_case(7, 200, uc.REL)
    eng.set_usage_tables(tab)

    def answers():
        p = eng.probe(probes)
        code, counts = eng.commit_check(None, abi.CommitJobs(time_limit_sec=jobs.time_limit_sec))
        nf, of, clean = eng.release_usage(rows)
        return p, code.copy(), counts.copy(), nf.copy(), of.copy(), clean

    a = answers()
    eng.advance_running([1000, 1001], now, 50000 + np.arange(jobs.num_jobs))
    b = answers()
    assert a[0].diff(b[0]) is None and all(np.array_equal(x, y) for x, y in zip(a[1:5], b[1:5])) and a[5] == b[5]
    eng.close()
