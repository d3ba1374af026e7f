"""The C++ adapter (GpuNodeSelectionAlgo, cranesched_amd/host) against the oracle, job by job, through the string-keyed objects CraneCtld
hands it.  tests/adapter_case.py builds the cases, derives the ABI arrays from the reference's rules on its own and turns oracle
placements into the objects NodeSelect must leave behind.

Without a device: the adapter's packed arrays (PackedArraysForTest) == the derived arrays, and its write-back of the oracle's placements
(WriteBackForTest) == the expected objects, under every write-back mode.  On the GPU: NodeSelect end to end == the oracle, on one engine
and on a group of two, with the event-fed mirror, a batch limit, empty queues and a second cycle after a drain flip."""
import pytest

from cranesched_amd import synth

from tests import adapter_case as A
from tests import helpers
from tests.test_overlap import overlap_case
from tests.test_reservations import random_resv_case

MODES = ["lazy", "full", "deferred"]


def make_case(kind: str, seed: int):
    if kind == "random":
        c, j, now, run = helpers.random_case(seed, N=48, J=240)
        return A.to_case(c, j, now, run, seed=seed)
    if kind == "resv":
        c, j, now, run, rv = random_resv_case(seed, N=40, J=240)
        return A.to_case(c, j, now, run, rv, seed=seed)
    if kind == "overlap":
        c, j, now, run = overlap_case(seed, N=48, J=240)
        return A.to_case(c, j, now, run, seed=seed)
    if kind in ("C3", "C4", "C5"):   # the benchmark configs, scaled down
        c, j, now = synth.make_config(kind, J=3000, N=256, P=1 if kind == "C3" else 4)
        return A.to_case(c, j, now, None, seed=seed)
    if kind == "C4r":
        c, j, now, run = synth.make_loaded("C4r", J=3000, N=256, P=4)
        return A.to_case(c, j, now, run, seed=seed)
    raise ValueError(kind)


CPU_CASES = [("random", s) for s in range(20)] + [("resv", s) for s in range(3)] + [("overlap", s) for s in range(2)] + \
            [("C3", 0), ("C4r", 0)]


def _pack_and_check(tmp_path, case, d):
    cf, pf = tmp_path / "case.txt", tmp_path / "pack.txt"
    case.write(cf)
    A.run_driver(["--case-pack", cf, pf])
    A.compare_pack(A.read_pack(pf), d)
    return cf


def _compare_objects(got, exp, tag):
    assert len(got) == len(exp), f"{tag}: {len(got)} jobs dumped, {len(exp)} expected"
    for g, e in zip(got, exp):
        assert g == e, f"{tag}: job {e['job']} differs\nadapter:  {g}\nexpected: {e}"


def test_cases_set_every_trap():
    """The generator must keep the traps it promises, or the tests below check less than they say."""
    case = make_case("resv", 0)
    names = [n["name"] for n in case.nodes]
    assert names != sorted(names) and any(int(a[2:]) > int(b[2:]) for a, b in zip(names, names[1:]))
    d = A.derive(case)
    widths = dict(zip(d.classes, d.layout.class_width))
    slots = sorted({s for (n, t, s) in d.slot_bit if (n, t) == d.classes[0]})
    assert widths[d.classes[0]] > 10 and slots != sorted(slots, key=lambda s: int(s.rsplit("nvidia", 1)[1]))
    assert len([c for c in d.classes if c[0] == "gpu"]) >= 2
    assert all(n["res"]["msw"] != n["res"]["mem"] for n in case.nodes)
    assert any(not n["alive"] for n in case.nodes) and any(n["drain"] for n in case.nodes)
    in_part = {x for _, lst in case.partitions for x in lst}
    assert any(n not in in_part for n in names)
    pend = case.pending
    assert any(p["node_req"]["msw"] != p["node_req"]["mem"] for p in pend)
    assert any(x not in names for p in pend for x in p["incl"]) and any(x not in names for p in pend for x in p["excl_nodes"])
    assert any(x in names and x not in in_part for p in pend for x in p["incl"])
    assert any(p["partition"] == "nopart" for p in pend) and any(p["resv"] == "noresv" for p in pend)
    assert any("tpu" in p["node_req"]["gres"] for p in pend)
    assert any("v100" in p["node_req"]["gres"].get("gpu", (0, {}))[1] for p in pend)
    assert any(p["reason"] == "License" for p in make_case("random", 3).pending)


@pytest.mark.parametrize("kind,seed", CPU_CASES)
def test_pack_and_write_back_match_the_derivation(built, tmp_path, kind, seed):
    """PackedArraysForTest == the derived arrays; WriteBackForTest(oracle placements) == the expected objects, in every mode"""
    case = make_case(kind, seed)
    d = A.derive(case)
    cf = _pack_and_check(tmp_path, case, d)
    pl = A.oracle_select(d, case.now)
    pf, of = tmp_path / "placements.txt", tmp_path / "objects.txt"
    A.write_placements(pl, pf)
    for mode in MODES:
        A.run_driver(["--case-write-back", cf, pf, of, "--write-back", mode])
        got, _ = A.read_dump(of)
        _compare_objects(got, A.expected(case, d, pl, mode), f"{kind}/{seed}/{mode}")


def test_a_request_for_an_absent_gres_name_never_fits_whatever_the_map_order(built, tmp_path):
    """A GresMap entry for a name no node carries marks the job as never fitting; another, known name of the same request must not
    overwrite that mark, whichever order the unordered_map hands them out in."""
    c, j, now, run = helpers.random_case(1, N=24, J=60)
    case = A.to_case(c, j, now, run, seed=1, traps=False)
    for p in case.pending:
        p["node_req"]["gres"] = {"tpu": (1, {}), "gpu": (1, {}), "npu": (1, {})}
    d = A.derive(case)
    assert (d.jobs.gres_total[:, 0] == 255).all()
    _pack_and_check(tmp_path, case, d)


# ---- on the GPU: NodeSelect end to end --------------------------------------------------------------------------------------------------

def _gpu_cycle(tmp_path, case, mode="lazy", devices="0", batch=0, mirror=False, then=None, tag=""):
    cf, of = tmp_path / "case.txt", tmp_path / "out.txt"
    case.write(cf)
    args = ["--case-file", cf, of, "--write-back", mode, "--devices", devices]
    if batch:
        args += ["--batch", batch]
    if mirror:
        args += ["--mirror"]
    if then is not None:
        cf2, of2 = tmp_path / "case2.txt", tmp_path / "out2.txt"
        then.write(cf2)
        args += ["--then", cf2, of2]
    A.run_driver(args, timeout=300)
    outs = [A.read_dump(of)] + ([A.read_dump(tmp_path / "out2.txt")] if then is not None else [])
    preempting = []   # m_preempting_set_ lives in the adapter object across its cycles
    for k, (got, tail) in zip((case, then), outs):
        d = A.derive(k, running_order="id" if mirror else "case", preempting=preempting)
        pl, po = A.oracle_select(d, k.now, batch, with_preempt=True)
        assert tail is not None and tail["status"] == 0, f"{tag}: {tail}"
        assert tail["refused"] == []
        if po is None:
            assert tail["cancel"] == [] and tail["preempting"] == []
        else:   # LastPreemptCancel (EnqueuePreemptCancel's list, cpp:6793) and PreemptingSet (m_preempting_set_)
            assert tail["cancel"] == po.cancelled_ids(), f"{tag}: cancel {tail['cancel']} vs oracle {po.cancelled_ids()}"
            assert tail["preempting"] == sorted(po.preempting_ids()), f"{tag}: preempting set {tail['preempting']} vs {po.preempting_ids()}"
            preempting = tail["preempting"]
        _compare_objects(got, A.expected(k, d, pl, mode, po), tag)
        from oracle import pyoracle
        if pyoracle.ref_available():   # the reference's own code (oracle/_ref) as a second checker, as smoke() does
            pr, ppo = A.oracle_select(d, k.now, batch, backend="ref", with_preempt=True)
            assert pr.diff(pl) is None, f"{tag}: the oracle and the reference's own code differ: {pr.diff(pl)}"
            if po is not None:
                assert ppo.lists() == po.lists() and ppo.cancelled_ids() == po.cancelled_ids(), f"{tag}: preemption differs from the reference's own code"
    return outs


GPU_CASES = [("random", 0), ("random", 5), ("resv", 1), ("overlap", 0)]


@pytest.mark.gpu
@pytest.mark.parametrize("devices", ["0", "0,0"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind,seed", GPU_CASES)
def test_node_select_matches_the_oracle(built, tmp_path, kind, seed, mode, devices):
    _gpu_cycle(tmp_path, make_case(kind, seed), mode=mode, devices=devices, tag=f"{kind}/{seed}/{mode}/{devices}")


@pytest.mark.gpu
@pytest.mark.parametrize("kind,seed", GPU_CASES)
def test_node_select_on_the_event_fed_mirror_matches_the_oracle(built, tmp_path, kind, seed):
    _gpu_cycle(tmp_path, make_case(kind, seed), mode="full", mirror=True, tag=f"mirror {kind}/{seed}")


@pytest.mark.gpu
@pytest.mark.parametrize("devices", ["0", "0,0"])
@pytest.mark.parametrize("batch", [1, 57, 239])
def test_node_select_with_a_batch_limit_matches_the_oracle(built, tmp_path, devices, batch):
    _gpu_cycle(tmp_path, make_case("random", 2), mode="full", devices=devices, batch=batch, tag=f"batch {batch}/{devices}")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["C3", "C4", "C5", "C4r"])
def test_scaled_benchmark_configs_match_the_oracle(built, tmp_path, kind):
    _gpu_cycle(tmp_path, make_case(kind, 0), mode="deferred", devices="0,0" if kind == "C4" else "0", tag=kind)


def _empty(case):
    e = A.Case(case.now)
    e.nodes, e.partitions, e.resvs, e.running = case.nodes, case.partitions, case.resvs, case.running
    return e


def _next_cycle(case, first_objects, dt=30):
    """What CraneCtld hands the next cycle: the jobs that started become running jobs (with the allocation NodeSelect gave them), the
    others are pending again as fresh objects, and one schedulable node is drained."""
    nxt = A.Case(case.now + dt)
    nxt.partitions, nxt.resvs = case.partitions, case.resvs
    nxt.nodes = [dict(n) for n in case.nodes]
    flip = next(i for i, n in enumerate(nxt.nodes) if n["alive"] and not n["drain"])
    nxt.nodes[flip]["drain"] = True
    nxt.running = list(case.running)
    for p, o in zip(case.pending, first_objects):
        if o["reason"] == "" and o["start"] == case.now:
            res = {cid: {k: a[k] for k in ("cpu", "mem", "msw", "cores", "gres")} for cid, a in o["alloc"].items()}
            nxt.running.append({"id": p["id"], "qos": p["qos"], "qos_priority": 0, "resv": p["resv"], "start": o["start"], "end": o["end"],
                                "res": res})
        else:
            nxt.pending.append(p)
    return nxt


@pytest.mark.gpu
@pytest.mark.parametrize("mirror", [False, True])
@pytest.mark.parametrize("kind,seed", [("random", 7), ("resv", 2)])
def test_a_second_cycle_after_a_drain_flip_matches_the_oracle(built, tmp_path, kind, seed, mirror):
    case = make_case(kind, seed)
    d = A.derive(case, running_order="id" if mirror else "case")
    first = A.expected(case, d, A.oracle_select(d, case.now), "full")
    nxt = _next_cycle(case, first)
    assert len(nxt.running) > len(case.running) and nxt.pending
    _gpu_cycle(tmp_path, case, mode="full", mirror=mirror, then=nxt, tag=f"two cycles {kind}/{seed} mirror={mirror}")


@pytest.mark.gpu
@pytest.mark.parametrize("devices", ["0", "0,0"])
def test_an_empty_queue_as_the_first_cycle_and_after_a_full_one(built, tmp_path, devices):
    """An empty first cycle leaves the adapter's job vectors unfilled (null data()); a group of engines must accept that as one engine
    does, and the object must serve the cycles after it."""
    case = make_case("random", 4)
    empty = _empty(case)
    (tmp_path / "a").mkdir()
    (got, tail), = _gpu_cycle(tmp_path / "a", empty, devices=devices, tag=f"empty first/{devices}")
    assert got == [] and tail["status"] == 0
    (tmp_path / "b").mkdir()
    _gpu_cycle(tmp_path / "b", empty, devices=devices, then=case, tag=f"empty then full/{devices}")
    (tmp_path / "c").mkdir()
    _gpu_cycle(tmp_path / "c", case, devices=devices, then=_empty(case), tag=f"full then empty/{devices}")


# ---- preemption: NodeSelect(now, running, pending) with a QoS table, against the oracle's PreemptOut -------------------------------------

def preempt_case(seed: int):
    from tests.test_preempt import random_preempt_case
    c, j, now, run, pre = random_preempt_case(seed, N=12, J=90, P=2, running=24)
    return A.to_case(c, j, now, run, seed=seed, pre=pre)


def test_preempt_cases_preempt():
    """the generator must actually exercise the path: preempted running and pending jobs, a cancel list, an unknown QoS"""
    kinds, cancels = set(), 0
    for seed in range(6):
        case = preempt_case(seed)
        d = A.derive(case)
        pl, po = A.oracle_select(d, case.now, with_preempt=True)
        kinds |= {is_pd for lst in po.lists() for is_pd, _ in lst}
        cancels += len(po.cancelled_ids())
        assert any(p["qos"] == "guest" for p in case.pending) and any(r["qos"] == "guest" for r in case.running)
    assert kinds == {False, True} and cancels >= 2


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("seed", range(6))
def test_preemption_matches_the_oracle(built, tmp_path, seed, mode):
    """QoS names -> ids, priorities and start times as TryPreempt_ reads them; preempted_jobs (kind, job id) in push order, a pending
    job preempted in the cycle with reason "Preempted", LastPreemptCancel and PreemptingSet == the oracle's PreemptOut"""
    _gpu_cycle(tmp_path, preempt_case(seed), mode=mode, tag=f"preempt {seed}/{mode}")


@pytest.mark.gpu
def test_preemption_carries_the_preempting_set_into_the_next_cycle(built, tmp_path):
    case = preempt_case(2)
    d = A.derive(case)
    first = A.expected(case, d, *A.oracle_select(d, case.now, with_preempt=True)[:1], "full")
    _gpu_cycle(tmp_path, case, mode="full", then=_next_cycle(case, first), tag="preempt two cycles")


@pytest.mark.gpu
def test_preemption_over_two_devices_is_refused_loudly(built, tmp_path):
    """a cycle with preemption runs on ONE device (NodeSelectionAlgo.cpp): over 0,0 every job not already held back leaves with
    "GpuEngineError" and nothing else, and the status says why"""
    case = preempt_case(0)
    cf, of = tmp_path / "case.txt", tmp_path / "out.txt"
    case.write(cf)
    A.run_driver(["--case-file", cf, of, "--devices", "0,0"])
    got, tail = A.read_dump(of)
    assert tail["status"] != 0 and "ONE device" in tail["error"]
    for g, p in zip(got, case.pending):
        assert g["reason"] == (p["reason"] or "GpuEngineError") and g["start"] == 0 and g["craned_ids"] == [] and g["preempted"] == []


# ---- hand-built cases, one per trap: a small cluster, every job hit by the same trap ------------------------------------------------------

def _small(seed=11):
    c, j, now, run = helpers.random_case(seed, N=24, J=80, P=2, running=12)
    return A.to_case(c, j, now, run, seed=seed, traps=False)


def _trap(name):
    case = _small()
    names = [n["name"] for n in case.nodes]
    orphan = {"name": "cn0", "alive": True, "drain": False,
              "res": {"cpu": 64 * 256, "mem": 256 * A.GIB, "msw": 5 * A.GIB, "cores": list(range(64)), "gres": {}}}
    if name == "unknown include node":
        for p in case.pending: p["incl"] = [names[3], "ghost"]
    elif name == "include outside the partition":
        case.nodes.append(orphan)
        for p in case.pending: p["incl"] = ["cn0"] + case.partitions[0][1][:2]
    elif name == "unknown exclude node":
        for p in case.pending: p["excl_nodes"] = ["ghost", names[5]]
    elif name == "unknown partition":
        for x, p in enumerate(case.pending):
            if x % 2: p["partition"] = "nopart"
    elif name == "unknown reservation":
        for x, p in enumerate(case.pending):
            if x % 2: p["resv"] = "noresv"
    elif name == "absent gres name":
        for p in case.pending: p["node_req"]["gres"] = {"tpu": (1, {}), **p["node_req"]["gres"]}
    elif name == "absent gres type":
        for p in case.pending: p["node_req"]["gres"] = {"gpu": (1, {"v100": 1})}
    elif name == "preset reason":
        for x, p in enumerate(case.pending):
            if x % 3 == 0: p["reason"] = "License"
    elif name == "dead and drained nodes":
        for x, n in enumerate(case.nodes):
            n["alive"], n["drain"] = x % 4 != 1, x % 4 == 2
    elif name == "memory_sw":
        for x, p in enumerate(case.pending):
            p["excl"] = x % 3 == 0
            p["node_req"]["msw"], p["task_req"]["msw"] = 7 * A.GIB + x, 3 * A.GIB + x
    elif name == "node in no partition":
        case.nodes.insert(0, orphan)
    elif name == "slot ids > 10, string order":
        pass   # every case built by to_case: /dev/nvidia0..11 in one class of two types under "gpu"
    return case


TRAPS = ["unknown include node", "include outside the partition", "unknown exclude node", "unknown partition", "unknown reservation",
         "absent gres name", "absent gres type", "preset reason", "dead and drained nodes", "memory_sw", "node in no partition",
         "slot ids > 10, string order"]


@pytest.mark.parametrize("trap", TRAPS)
def test_each_trap_alone(built, tmp_path, trap):
    case = _trap(trap)
    d = A.derive(case)
    cf = _pack_and_check(tmp_path, case, d)
    pl = A.oracle_select(d, case.now)
    pf, of = tmp_path / "placements.txt", tmp_path / "objects.txt"
    A.write_placements(pl, pf)
    for mode in MODES:
        A.run_driver(["--case-write-back", cf, pf, of, "--write-back", mode])
        got, _ = A.read_dump(of)
        _compare_objects(got, A.expected(case, d, pl, mode), f"{trap}/{mode}")


# ---- the full-size C4 cycle through the adapter ------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_full_size_c4_through_the_adapter_matches_the_golden_digest(built, tmp_path):
    """1 M jobs x 64 k nodes through SetClusterSnapshot / NodeSelect (full write-back): the objects, mapped back to placement records
    through the snapshot's name -> index map, give the oracle's full-run digest (tests/golden/fullrun_c4.npz) — every job's start,
    reason and records, per 10 000 jobs, and the reason counts.  (Costs and time maps are not visible through the adapter; the
    engine-level full-run test compares those.)  The driver prints NodeSelect's wall time."""
    import os
    import numpy as np
    from cranesched_amd import abi
    from tests import fullrun
    from tests.golden.make_fullrun import CASES, load_case5
    ref = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fullrun_c4.npz")))
    name, J, N, P = CASES["c4"]
    cluster, jobs, now, running, pre = load_case5(name, J, N, P)
    assert running is None and pre is None
    case = A.to_case(cluster, jobs, now, None, plain=True)
    cf, of, sf = tmp_path / "case.txt", tmp_path / "out.txt", tmp_path / "soa.bin"
    case.write(cf)
    r = A.run_driver(["--case-file", cf, of, "--write-back", "full", "--soa-out", sf], timeout=900)
    print(r.stdout.strip().splitlines()[0])
    Jn = jobs.num_jobs
    raw = open(sf, "rb").read()
    pl = abi.Placements(Jn, jobs.total_places())
    pos = 0
    for f, dt, n in (("start_sec", np.int64, Jn), ("reason", np.uint8, Jn), ("place_offsets", np.uint64, Jn + 1)):
        getattr(pl, f)[:n] = np.frombuffer(raw, dt, n, pos); pos += n * np.dtype(dt).itemsize
    M = int(pl.place_offsets[Jn])
    assert M == pl.capacity
    for f, dt in (("node_idx", np.uint32), ("ntasks", np.uint32), ("cpu_raw", np.int64), ("mem", np.uint64), ("core_lo", np.uint64),
                  ("core_hi", np.uint64), ("gres", np.uint64)):
        getattr(pl, f)[:M] = np.frombuffer(raw, dt, M, pos); pos += M * np.dtype(dt).itemsize
    assert pos == len(raw)
    got = fullrun.digest(pl, np.zeros(1, np.uint64), lambda n: {k: np.zeros(0) for k in ("t", "cpu_raw", "mem", "core_lo", "core_hi", "gres")}, 1)
    assert np.array_equal(got["counts"], ref["counts"]), f"reason counts {got['counts'].tolist()} vs {ref['counts'].tolist()}"
    ne = np.nonzero(got["chunk_crc"] != ref["chunk_crc"])[0]
    assert len(ne) == 0, f"{len(ne)} of {len(ref['chunk_crc'])} job chunks differ, first = jobs [{ne[0] * fullrun.CHUNK}, ...)"
