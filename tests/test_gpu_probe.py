"""What-if probes (include/crane_gpu_probe/probe.h, csrc/probe_kernel.inc) on the GPU against tests/probe_case.expected: per probe ONE
oracle cycle over `ordered jobs + [probe]`, result of the last job.  Parity is run behind every selection kernel (engine_cls; the
k_mem and k_giant widths in cases of their own): the state a probe reads has the same layout whichever kernel produced it, and this
is where a front array left stale by one of them would show.  Also: the model is read-only under a probe call, the state machine
of the calls, a probe into a refused partition.

The expected answers are computed once per scenario and shared by the kernels' runs (they do not depend on the kernel)."""
import dataclasses
import functools
import time

import numpy as np
import pytest

from cranesched_amd import abi, synth
from cranesched_amd.engine import EngineError
from oracle import pyoracle
from tests import helpers
from tests import probe_case as pc

pytestmark = pytest.mark.gpu


# ---- scenarios: name -> (cluster, jobs, probes, now, running, reservations, engine config) ----------------------------------------
def _synth_probes(name, Q, P, seed):
    """Q jobs of config `name`'s generator with another seed."""
    cfg = synth.CONFIGS[name]
    return synth.make_jobs(Q, P, cfg["gres"], synth.SEED0 ^ seed, cfg["Q"], cfg["LM"])


@functools.lru_cache(maxsize=None)
def scenario(name):
    rv, cfg = None, {}
    if name.startswith("random"):
        c, j, p, now, run = pc.random_scenario(int(name[6:]))
    elif name == "wide_cores":
        c, j, p, now, run = pc.random_scenario(2)
        c = helpers.widen_cores(c, 2)
    elif name == "plain_shapes":          # no ntasks > node_num, no node lists
        c, j, p, now, run = pc.random_scenario(3, general=False, lists=False)
    elif name == "resv":
        c, j, p, now, run, rv = pc.resv_scenario(0)
    elif name.startswith("overlap"):
        c, j, p, now, run = pc.overlap_scenario(1, layout={"overlap": "all+subsets", "overlap_chain": "chain", "overlap_random": "random"}[name])
    elif name == "reserved_kat":
        c, j, p, now, run, rv, _ = pc.reserved_kat()
    elif name == "loaded":                # a loaded cluster (running jobs on every node, deep time maps): C4r scaled
        c, j, now, run = synth.make_loaded("C4r", J=3000, N=1024, P=4)
        p = _synth_probes("C4", 40, 4, 0x9901)
    elif name == "batch":                 # scheduled_batch_size = J / 2: the probes see the state after the jobs the loop took
        c, j, p, now, run = pc.random_scenario(1)
        cfg = {"scheduled_batch_size": j.num_jobs // 2}
    elif name == "full_nodes":            # max_job_num_per_node = 12 on a deep queue: nodes whose FINAL map is full are skipped (:6194)
        c, j, now = synth.make_config("C2", J=1500, N=16, P=1)
        run = None
        p = _synth_probes("C2", 24, 1, 0x9902)
        cfg = {"max_job_num_per_node": 12}
    else:
        raise KeyError(name)
    return c, j, p, now, run, rv, cfg


@functools.lru_cache(maxsize=None)
def expected_of(name):
    c, j, p, now, run, rv, cfg = scenario(name)
    t0 = time.time()
    kw = {k: v for k, v in cfg.items() if k != "scheduled_batch_size"}
    exp = pc.expected(c, j, p, now, running=run, reservations=rv, batch=cfg.get("scheduled_batch_size", 0), **kw)
    print(f"expected({name}): {p.num_jobs} oracle cycles of {j.num_jobs} + 1 jobs in {time.time() - t0:.1f} s")
    return exp


def _cycle(engine_cls, c, j, now, run, rv, cfg):
    eng = engine_cls(device=0, **cfg)
    eng.set_nodes(c)
    if rv is not None:
        eng.set_reservations(rv)
    if run is not None:
        eng.set_running(run)
    got = eng.node_select(now, j)
    return eng, got


def _assert_probes(tag, got, exp, probes):
    d = got.diff(exp)
    if d is not None and isinstance(d[1], int):
        f, i = d[0], d[1]
        q = i if f in ("start_sec", "reason") else int(np.searchsorted(exp.place_offsets[:probes.num_jobs + 1], i, side="right") - 1)
        raise AssertionError(f"{tag}: probe {q} differs from the oracle in {d}; node_num {probes.node_num[q]} ntasks {probes.ntasks[q]} "
                             f"expected start {exp.start_sec[q]} reason {exp.reason[q]}, got start {got.start_sec[q]} reason {got.reason[q]}")
    assert d is None, f"{tag}: {d}"


PARITY = ["random0", "random1", "random2", "random3", "random4", "random5", "wide_cores", "plain_shapes", "resv", "overlap", "overlap_chain",
          "overlap_random", "reserved_kat", "loaded", "batch", "full_nodes"]


@pytest.mark.parametrize("name", PARITY)
def test_probe_parity(engine_cls, name):
    c, j, p, now, run, rv, cfg = scenario(name)
    exp = expected_of(name)
    eng, got_cycle = _cycle(engine_cls, c, j, now, run, rv, cfg)
    try:
        # the cycle itself is the oracle's (else a probe mismatch would say nothing about the probe path)
        ref = pyoracle.select(c, j, now, running=run, reservations=rv, **cfg)
        assert got_cycle.diff(ref.placements) is None, f"{name}: the cycle differs from the oracle"
        got = eng.probe(p)
        _assert_probes(f"{name} behind {eng.last_kernel()}", got, exp, p)
    finally:
        eng.close()


def test_coverage_of_the_random_scenarios(built):
    """Asserted on the ORACLE's answers: the parity cases ask hard questions too."""
    mix = {}
    for s in pc.RANDOM_SEEDS:
        c, j, p, now, run, rv, cfg = scenario(f"random{s}")
        mix = pc.add_mix(mix, pc.outcome_mix(expected_of(f"random{s}"), p, now))
    print("outcome mix:", mix)
    pc.check_mix(mix)
    _, _, p, now, _, _, _ = scenario("reserved_kat")
    assert pc.outcome_mix(expected_of("reserved_kat"), p, now)["reserved"] == 1, "a 'Resource Reserved' probe"
    r = expected_of("resv").reason[:pc.Q_RANDOM]
    assert (r == abi.REASON_RESERVATION_NOT_FOUND).sum() > 0
    c, j, p, now, run, rv, cfg = scenario("full_nodes")
    loose = pc.expected(c, j, p, now)
    assert expected_of("full_nodes").diff(loose) is not None, "max_job_num_per_node must bind for some probe of full_nodes"


# ---- the k_mem and k_giant widths ---------------------------------------------------------------------------------------------
def _wide_case(engine_default, c, j, p, now, want_kernel, tag):
    t0 = time.time()
    exp = pc.expected(c, j, p, now)
    cpu_s = time.time() - t0
    eng, got_cycle = _cycle(engine_default, c, j, now, None, None, {})
    try:
        k = eng.last_kernel()
        assert want_kernel in k, (tag, k)
        ref = pyoracle.select(c, j, now)
        assert got_cycle.diff(ref.placements) is None, f"{tag}: the cycle differs from the oracle"
        got = eng.probe(p)
        print(f"{tag}: {p.num_jobs} probes behind {k}; expected() took {cpu_s:.1f} s on the CPU; k_probe {eng.probe_timing()['kernel_ms']:.2f} ms")
        _assert_probes(tag, got, exp, p)
        m = pc.outcome_mix(exp, p, now)
        assert m["now"] + m["later"] >= 4, m
    finally:
        eng.close()


def test_probe_behind_k_giant(engine_default):
    """One partition of 131 072 nodes (k_giant).  8 probes: 8 oracle cycles of 1 500 + 1 jobs over 131 072 nodes, ~10 s on the CPU."""
    c, j, now = synth.make_config("C4", J=1500, N=131_072, P=1)
    p = _synth_probes("C4", 8, 1, 0x9903)
    _wide_case(engine_default, c, j, p, now, "k_giant", "one partition of 131 072 nodes")


def test_probe_behind_k_mem_on_a_shared_group(engine_default):
    """C4 plus an ALL partition over all 65 536 nodes: one group of 131 072 slots on k_mem; the probes go to ALL and to the subsets (own
    slot range, own cost, the node's one time map).  8 probes: 8 oracle cycles of 1 500 + 1 jobs, ~10 s on the CPU."""
    c, j, now = synth.make_mixed("C4all64k", J=1500)[:3]
    p = _synth_probes("C4", 8, 8, 0x9904)
    part = p.partition.copy()
    part[::2] = c.num_partitions - 1     # every second probe into ALL
    p.partition = part.astype(np.uint32)
    _wide_case(engine_default, c, j, p, now, "k_mem", "ALL over 65 536 nodes")


# ---- read-only, repeatable, order-free ------------------------------------------------------------------------------------------
def _snapshot(eng, c, got):
    nodes = np.unique(np.linspace(0, c.num_nodes - 1, 24).astype(np.int64))
    in_part = np.zeros(c.num_nodes, bool)
    in_part[np.asarray(c.part_nodes, np.int64)] = True
    tl = {int(n): {k: v.copy() for k, v in eng.timeline(int(n)).items()} for n in nodes if in_part[n]}
    return eng.costs().view(np.uint64).copy(), tl, eng.download(), dict(eng.timing())


def test_probe_is_read_only_repeatable_and_order_free(engine_cls):
    c, j, p, now, run, rv, cfg = scenario("random4")
    exp = expected_of("random4")
    eng, got_cycle = _cycle(engine_cls, c, j, now, run, rv, cfg)
    try:
        costs0, tl0, dl0, tm0 = _snapshot(eng, c, got_cycle)
        a = eng.probe(p)
        costs1, tl1, dl1, tm1 = _snapshot(eng, c, got_cycle)
        assert np.array_equal(costs0, costs1), "costs changed under a probe call"
        for n in tl0:
            for f in tl0[n]:
                assert np.array_equal(tl0[n][f], tl1[n][f]), f"time map of node {n} changed under a probe call ({f})"
        assert dl0.diff(dl1) is None and dl1.diff(got_cycle) is None, "the cycle's results changed under a probe call"
        for f in ("h2d_ms", "init_ms", "select_ms", "jobs_ordered", "algorithmic_bytes"):
            assert tm0[f] == tm1[f], f"cns_get_timing().{f} changed under a probe call"
        b = eng.probe(p)
        assert a.diff(b) is None, "the same probes twice"
        _assert_probes("first call", a, exp, p)
        Q = p.num_jobs
        rev = eng.probe(pc.take(p, np.arange(Q)[::-1]))
        back = abi.Placements(Q, p.total_places())
        back.place_offsets[:] = a.place_offsets
        for i in range(Q):
            r = Q - 1 - i
            back.start_sec[i], back.reason[i] = rev.start_sec[r], rev.reason[r]
            s0, s1, d0 = int(rev.place_offsets[r]), int(rev.place_offsets[r + 1]), int(a.place_offsets[i])
            for f in ("node_idx", "ntasks", "cpu_raw", "mem", "core_lo", "core_hi", "gres", "core_w2", "core_w3"):
                getattr(back, f)[d0:d0 + s1 - s0] = getattr(rev, f)[s0:s1]
        assert back.diff(a) is None, "probes reversed -> answers reversed"
        # Q = 0 and Q = 1
        none = eng.probe(pc.take(p, []))
        assert none.num_jobs == 0
        one = eng.probe(pc.take(p, [7]))
        assert one.start_sec[0] == a.start_sec[7] and one.reason[0] == a.reason[7]
        s0, s1 = int(a.place_offsets[7]), int(a.place_offsets[8])
        assert np.array_equal(one.node_idx[:s1 - s0], a.node_idx[s0:s1]) and np.array_equal(one.cpu_raw[:s1 - s0], a.cpu_raw[s0:s1])
        # ... and the cycle can still be run again with the same result
        assert eng.node_select(now, j).diff(got_cycle) is None
    finally:
        eng.close()


def test_more_probes_than_resident_workgroups(engine_default):
    """Q = 5 000 on a small cluster — more probes than workgroups the device holds at once, so the counter hands out several probes
    per workgroup — compared with the same probes asked 50 at a time; the first 50 against the oracle."""
    c, j, now, run = helpers.random_case(6)
    big = helpers.random_case(2006, J=5000)[1]
    eng, _ = _cycle(engine_default, c, j, now, run, None, {})
    try:
        all_at_once = eng.probe(big)
        off = all_at_once.place_offsets
        for lo in range(0, 5000, 50):
            part = eng.probe(pc.take(big, np.arange(lo, lo + 50)))
            assert np.array_equal(part.start_sec[:50], all_at_once.start_sec[lo:lo + 50]), lo
            assert np.array_equal(part.reason[:50], all_at_once.reason[lo:lo + 50]), lo
            a, b = int(off[lo]), int(off[lo + 50])
            for f in ("node_idx", "ntasks", "cpu_raw", "mem", "core_lo", "core_hi", "gres"):
                assert np.array_equal(getattr(part, f)[:b - a], getattr(all_at_once, f)[a:b]), (lo, f)
        first = pc.take(big, np.arange(50))
        _assert_probes("first 50 of 5 000", eng.probe(first), pc.expected(c, j, first, now, running=run), first)
    finally:
        eng.close()


# ---- one handle, two job tables ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _crossing_case(wide):
    """A 96-node cluster (optionally with nodes of 192 / 256 cores), queues of 40 and 3 jobs, probe tables of 5, 300 and 40, and the
    oracle's answer to every step of test_queue_and_probe_tables_cross_in_size."""
    c, j40, now, run = helpers.random_case(12, J=40)
    if wide:
        c = helpers.widen_cores(c, 12)
    j3 = pc.take(j40, [11, 4, 23])
    p300 = helpers.random_case(2008, J=300)[1]
    p5, p40 = pc.take(p300, np.arange(5)), pc.take(p300, np.arange(120, 160))
    ref40 = pyoracle.select(c, j40, now, running=run).placements
    ref3 = pyoracle.select(c, j3, now, running=run).placements
    exp = {"p5": pc.expected(c, j40, p5, now, running=run), "p300": pc.expected(c, j40, p300, now, running=run),
           "p40": pc.expected(c, j3, p40, now, running=run)}
    return c, now, run, j40, j3, {"p5": p5, "p300": p300, "p40": p40}, ref40, ref3, exp


@pytest.mark.parametrize("wide", [False, True], ids=["cores_to_128", "cores_to_256"])
def test_queue_and_probe_tables_cross_in_size(engine_default, wide):
    """The cycle's queue and the probes are two job tables on one handle, each with its buffers, counts and result layout.  Their sizes
    cross in both directions here (queue 40 > probes 5 and 0, probes 300 > queue 40, queue 3 < probes 40), so a step that reads the
    other table, or a capacity left from a larger one, is a wrong answer: every cycle against the oracle's, every probe table against
    tests/probe_case.expected, the cycle's download unchanged behind the probes, and the same again behind a refused cns_upload_jobs.
    Once more on a snapshot with core ids above 127: the core_w2 / core_w3 planes and their reset, for both tables."""
    c, now, run, j40, j3, p, ref40, ref3, exp = _crossing_case(wide)
    if wide:   # (asserted on the oracle's answers: the planes carry something in the first cycle and in the probes, nothing in the J = 3 cycle behind it)
        assert ref40.core_w3.any() and not ref3.core_w2.any() and exp["p5"].core_w3.any() and exp["p300"].core_w3.any() and exp["p40"].core_w2.any()
    eng = engine_default(device=0)
    try:
        eng.set_nodes(c)
        eng.set_running(run)
        first = eng.node_select(now, j40)
        assert first.diff(ref40) is None, "J = 40: the cycle differs from the oracle"
        _assert_probes("Q = 5 behind J = 40", eng.probe(p["p5"]), exp["p5"], p["p5"])
        none = pc.take(p["p300"], [])
        assert eng.probe(none).num_jobs == 0
        eng.probe_upload(none)                  # ... and an empty table through the steps of a full one
        assert eng.probe_run_resident() == 0.0 and eng.probe_download().num_jobs == 0
        _assert_probes("Q = 300 behind J = 40", eng.probe(p["p300"]), exp["p300"], p["p300"])
        assert eng.download().diff(first) is None, "the cycle's results changed under a probe table larger than the queue"
        assert eng.node_select(now, j3).diff(ref3) is None, "J = 3 behind Q = 300: the cycle differs from the oracle"
        _assert_probes("Q = 40 behind J = 3", eng.probe(p["p40"]), exp["p40"], p["p40"])
        bad = dataclasses.replace(j3, node_num=np.zeros(3, np.uint32))
        with pytest.raises(EngineError) as ei:
            eng.upload_jobs(bad)
        assert ei.value.status == -1
        assert eng.node_select(now, j3).diff(ref3) is None, "J = 3 behind a refused upload: the cycle differs from the oracle"
        _assert_probes("Q = 40 behind a refused upload", eng.probe(p["p40"]), exp["p40"], p["p40"])
    finally:
        eng.close()


# ---- state machine ------------------------------------------------------------------------------------------------------------
def test_probe_state_machine(engine_default):
    c, j, p, now, run, rv, cfg = scenario("random0")
    eng = engine_default(device=0)
    try:
        def status_of(fn):
            with pytest.raises(EngineError) as ei:
                fn()
            return ei.value.status
        eng.set_nodes(c)
        eng.set_running(run)
        assert status_of(lambda: eng.probe(p)) == -5, "before a run: CNS_ERR_STATE"
        eng.upload_jobs(j)
        assert status_of(lambda: eng.probe(p)) == -5, "uploaded, not run"
        eng.run_resident(now)
        a = eng.probe(p)
        _assert_probes("after run_resident", a, expected_of("random0"), p)
        eng.set_running(run)
        assert status_of(lambda: eng.probe(p)) == -5, "after set_running"
        eng.node_select(now, j)
        assert eng.probe(p).diff(a) is None
        eng.set_nodes(c)
        assert status_of(lambda: eng.probe(p)) == -5, "after set_nodes"
        eng.set_running(run)
        eng.node_select(now, j)
        eng.probe_upload(p)
        ms = eng.probe_run_resident()
        assert ms > 0.0 and eng.probe_timing()["kernel_ms"] == ms
        assert eng.probe_download().diff(a) is None and eng.probe_run_resident() > 0.0 and eng.probe_download().diff(a) is None
        eng.node_select(now, j)
        assert status_of(eng.probe_run_resident) == -5, "a new cycle drops the uploaded probes"
        bad = dataclasses.replace(p, node_num=np.zeros(p.num_jobs, np.uint32))
        assert status_of(lambda: eng.probe(bad)) == -1, "validated like cns_upload_jobs"
        assert eng.probe(p).diff(a) is None, "a refused call leaves the handle usable"
    finally:
        eng.close()


def test_probe_after_a_preemption_cycle_is_unsupported(engine_default):
    from tests.test_preempt import random_preempt_case
    c, j, now, run, pre = random_preempt_case(503)
    eng = engine_default(device=0)
    try:
        eng.set_nodes(c)
        eng.set_running(run)
        eng.node_select_preempt(now, j, pre)
        with pytest.raises(EngineError) as ei:
            eng.probe(pc.take(j, np.arange(5)))
        assert ei.value.status == -4 and "preempt" in str(ei.value)
        got = eng.node_select(now, j)       # a plain cycle behind it serves probes again
        exp = pc.expected(c, j, pc.take(j, np.arange(5)), now, running=run)
        _assert_probes("plain cycle after a preemption cycle", eng.probe(pc.take(j, np.arange(5))), exp, pc.take(j, np.arange(5)))
        assert got.num_jobs == j.num_jobs
    finally:
        eng.close()


def test_probe_into_a_refused_partition(engine_default):
    """tests/test_gpu_refusal.py's 512-core node: partition 5 is refused; probes into it come back CNS_REASON_ENGINE_REFUSED, probes into
    the other partitions are exact (the oracle on the queue without the refused jobs, which never reach an ordered loop)."""
    cluster, jobs, now = synth.make_config("C4", J=4000, N=1024, P=8)
    unsup = np.zeros(cluster.num_nodes, np.uint8)
    unsup[int(cluster.part_nodes[cluster.part_offsets[5] + 17])] = 1
    c2 = dataclasses.replace(cluster, unsupported=unsup)
    p = _synth_probes("C4", 48, 8, 0x9905)
    eng, _ = _cycle(engine_default, c2, jobs, now, None, None, {})
    try:
        assert eng.partition_status().tolist() == [0, 0, 0, 0, 0, 1, 0, 0]
        got = eng.probe(p)
        into5 = p.partition == 5
        assert into5.sum() >= 2 and (~into5).sum() >= 20
        assert (got.reason[:48][into5] == abi.REASON_ENGINE_REFUSED).all() and (got.start_sec[:48][into5] == 0).all()
        keep = np.nonzero(~into5)[0]
        served = np.nonzero(jobs.partition != 5)[0]
        exp = pc.expected(cluster, pc.take(jobs, served), pc.take(p, keep), now)
        _assert_probes("served partitions", eng.probe(pc.take(p, keep)), exp, pc.take(p, keep))
        off = got.place_offsets
        for x, i in enumerate(keep):
            assert got.start_sec[i] == exp.start_sec[x] and got.reason[i] == exp.reason[x]
            assert np.array_equal(got.node_idx[int(off[i]):int(off[i + 1])], exp.node_idx[int(exp.place_offsets[x]):int(exp.place_offsets[x + 1])])
    finally:
        eng.close()
