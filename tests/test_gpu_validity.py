"""The validity check of a batch of submissions (include/crane_gpu_valid/validity.h, csrc/valid_kernels.inc) on the GPU against
tests/valid_pyref.py, the restatement of JobScheduler::CheckJobValidity's partition checks: code and eligible of every job, for equality
(all integers, no tolerance).  The hand-derived table, 20 seeds of the generator, the seams of the walk kernel read from
cns_validate_shape, the errors, independence from a cycle and probes, invalidation by cns_set_nodes, and partitions the cycle refuses.

The expected answers are computed once per case and shared."""
import functools

import numpy as np
import pytest

from cranesched_amd import abi
from cranesched_amd.engine import EngineError
from tests import valid_case as vc
from tests import valid_pyref as ref

pytestmark = pytest.mark.gpu
G, CORE = vc.G, vc.CORE


def _same(what, got, want_code, want_elig):
    code, elig = got
    bad = np.flatnonzero((code != want_code) | (elig != want_elig))
    assert len(bad) == 0, (f"{what}: {len(bad)} of {len(want_code)} jobs differ, first job {int(bad[0])}: got "
                           f"{abi.VALID_STR.get(int(code[bad[0]]), int(code[bad[0]]))} / {int(elig[bad[0]])}, want "
                           f"{abi.VALID_STR[int(want_code[bad[0]])]} / {int(want_elig[bad[0]])}")


def _engine(engine_default, cluster, resv=None):
    eng = engine_default(device=0)
    eng.set_nodes(cluster)
    if resv is not None:
        eng.set_reservations(resv)
    return eng


def test_hand_cases(engine_default):
    cl, resv, jobs, want_code, want_elig = vc.hand()
    eng = _engine(engine_default, cl, resv)
    try:
        _same("hand table", eng.validate_jobs(jobs), want_code, want_elig)
        _same("hand table (again)", eng.validate_jobs(jobs), want_code, want_elig)
    finally:
        eng.close()
    eng = _engine(engine_default, cl)                               # cns_set_reservations is optional: num_resv is 0
    try:
        _same("without reservations", eng.validate_jobs(jobs), *ref.check(cl, jobs, None))
    finally:
        eng.close()


@pytest.mark.parametrize("seed", vc.GPU_SEEDS)
def test_generated(engine_default, seed):
    cl, resv, jobs, want_code, want_elig = vc.generated(seed)
    eng = _engine(engine_default, cl, resv)
    try:
        _same(f"seed {seed}", eng.validate_jobs(jobs), want_code, want_elig)
    finally:
        eng.close()


# ---- the seams of the walk kernel --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _shape():
    from cranesched_amd import engine
    import ctypes as C
    a, b = C.c_uint32(0), C.c_uint32(0)
    assert engine.lib().cns_validate_shape(C.byref(a), C.byref(b)) == 0
    return a.value, b.value


def _seam_cluster(sizes, big_last=True):
    """Disjoint partitions of the given sizes over 4-core 8 GiB nodes; the LAST node of every partition has 16 cores and 64 GiB."""
    nodes, parts, n = [], [], 0
    for s in sizes:
        parts.append(list(range(n, n + s)))
        nodes += [(4, 8 * G, 0, 1, 0)] * s
        if s and big_last:
            nodes[-1] = (16, 64 * G, 0, 1, 0)
        n += s
    nodes.append((4, 8 * G, 0, 1, 0))                              # (a snapshot needs a node even when every partition here is empty)
    parts.append([n])
    return vc.make_cluster(nodes, parts)


@functools.lru_cache(maxsize=None)
def _node_seams():
    tile, _ = _shape()
    sizes = [tile - 1, tile, tile + 1, 2 * tile + 1, 0, 1, 63, 64, 65]
    cl = _seam_cluster(sizes)
    rows = []
    for p, s in enumerate(sizes):
        first = int(cl.part_offsets[p])
        rows.append(dict(p=p, tcpu=CORE, tmem=G))                                        # every node
        rows.append(dict(p=p, tcpu=CORE, tmem=G, k=max(s, 1), nt=max(s, 1)))             # ... all of them asked for
        rows.append(dict(p=p, tcpu=16 * CORE, tmem=G))                                   # the only eligible node is the last node of the last tile
        rows.append(dict(p=p, tcpu=16 * CORE, tmem=G, excl=[first + s - 1] if s else [0]))   # ... and it is excluded
        rows.append(dict(p=p, tcpu=CORE, tmem=G, incl=list(range(first, first + s)) + [first + s]))   # an include list as long as the partition (+ 1 outside)
        rows.append(dict(p=p, tcpu=16 * CORE, tmem=G, incl=list(range(first, first + s))[::-1] or [5]))   # ... unsorted, one entry fits
        rows.append(dict(p=p, tcpu=CORE, tmem=G, excl=list(range(first, first + s, 2)) or [7]))
    jobs = vc.make_jobs(rows)
    return (cl, jobs) + ref.check(cl, jobs, None)


def test_node_count_seams(engine_default):
    """Partitions of node_tile - 1, node_tile, node_tile + 1, 2 node_tile + 1, 0, 1, 63, 64 and 65 nodes; include lists longer than a tile."""
    tile, _ = _shape()
    cl, jobs, want_code, want_elig = _node_seams()
    assert int(np.diff(jobs.incl_offsets.astype(np.int64)).max()) > tile
    last = want_elig[2::7]
    assert last.tolist() == [1, 1, 1, 1, 0, 1, 1, 1, 1], "the restatement sees the one eligible node at the end of the last tile"
    eng = _engine(engine_default, cl)
    try:
        _same("node seams", eng.validate_jobs(jobs), want_code, want_elig)
    finally:
        eng.close()


@functools.lru_cache(maxsize=None)
def _job_seams():
    _, chunk = _shape()
    counts = [chunk - 1, chunk, chunk + 1, 0, 3]                    # jobs per partition; partition 3 gets none
    cl = _seam_cluster([5, 70, 9, 4, 2])
    rng = np.random.default_rng(7)
    rows = []
    for p, c in enumerate(counts):
        for i in range(c):
            r = dict(p=p, tcpu=int(rng.choice([1, 4, 16])) * CORE, tmem=int(rng.choice([1, 8, 64])) * G)
            if i % 5 == 0:
                r.update(k=2, nt=2)
            if i % 11 == 0:
                r["excl"] = [int(cl.part_offsets[p + 1]) - 1]
            rows.append(r)
    rows += [dict(p=77, tcpu=CORE, tmem=G)] * 2                     # ... and two jobs of no partition
    order = rng.permutation(len(rows))                             # the jobs of a partition are scattered over the queue
    jobs = vc.make_jobs([rows[i] for i in order])
    return (cl, jobs) + ref.check(cl, jobs, None)


def test_job_count_seams(engine_default):
    """job_chunk - 1, job_chunk, job_chunk + 1 jobs of a partition, none for one partition among several."""
    cl, jobs, want_code, want_elig = _job_seams()
    assert len(set(want_code.tolist())) >= 3
    eng = _engine(engine_default, cl)
    try:
        _same("job seams", eng.validate_jobs(jobs), want_code, want_elig)
    finally:
        eng.close()


# ---- errors ------------------------------------------------------------------------------------------------------------------------------
def _status(fn):
    with pytest.raises(EngineError) as e:
        fn()
    return e.value.status


def test_errors_and_empty_call(engine_default):
    cl, resv, jobs, want_code, want_elig = vc.hand()
    eng = engine_default(device=0)
    try:
        assert _status(lambda: eng.validate_jobs(jobs)) == -5                                  # before cns_set_nodes
        eng.set_nodes(cl)
        eng.set_reservations(resv)
        for lst in ("incl", "excl"):
            twice = vc.make_jobs([dict(p=0, tcpu=CORE, tmem=G), dict(p=0, tcpu=CORE, tmem=G, **{lst: [2, 0, 2]})])
            assert _status(lambda: eng.validate_jobs(twice)) == -1                             # a node twice in one list
            beyond = vc.make_jobs([dict(p=0, tcpu=CORE, tmem=G, **{lst: [900, 1, 900]})])
            assert _status(lambda: eng.validate_jobs(beyond)) == -1                            # ... also one that does not exist
        none = vc.make_jobs([])
        code, elig = np.full(4, 77, np.uint8), np.full(4, 77, np.uint32)
        eng.validate_jobs(none, out=(code, elig))                                              # num_jobs == 0: CNS_OK, nothing written
        assert (code == 77).all() and (elig == 77).all()
        _same("after the refusals", eng.validate_jobs(jobs), want_code, want_elig)
    finally:
        eng.close()


# ---- beside a cycle ----------------------------------------------------------------------------------------------------------------------
def test_independent_of_a_cycle_and_probes(engine_default):
    """A cycle, then validate, the same cycle again, probes, validate again: both cycles and both answers are identical."""
    from tests import probe_case as pc
    c, j, p, now, run, rv = pc.resv_scenario(0)
    want = ref.check(c, j, ref.resv_node_sets(rv))
    plain = engine_default(device=0)
    mixed = engine_default(device=0)

    def cycle(eng):
        eng.set_nodes(c)
        eng.set_reservations(rv)
        eng.set_running(run)
        return eng.node_select(now, j)

    try:
        want_sel = cycle(plain)
        want_costs = plain.costs().view(np.uint64).copy()
        want_probe = plain.probe(p)
        sel0 = cycle(mixed)
        assert sel0.diff(want_sel) is None and np.array_equal(mixed.costs().view(np.uint64), want_costs)
        first = mixed.validate_jobs(j)
        _same("behind a cycle", first, *want)
        assert mixed.download().diff(want_sel) is None, "the cycle's results behind the validity check"
        assert np.array_equal(mixed.costs().view(np.uint64), want_costs)
        sel1 = mixed.node_select(now, j)
        assert sel1.diff(want_sel) is None and np.array_equal(mixed.costs().view(np.uint64), want_costs)
        assert mixed.probe(p).diff(want_probe) is None
        second = mixed.validate_jobs(j)
        _same("behind a second cycle and probes", second, *want)
        assert np.array_equal(first[0], second[0]) and np.array_equal(first[1], second[1])
        assert mixed.probe(p).diff(want_probe) is None, "a probe behind the validity check"
    finally:
        plain.close()
        mixed.close()


def test_set_nodes_invalidates_the_tables(engine_default):
    cl, resv, jobs, want_code, want_elig = vc.hand()
    eng = _engine(engine_default, cl, resv)
    try:
        _same("before", eng.validate_jobs(jobs), want_code, want_elig)
        nodes = list(vc.HAND_NODES)
        nodes[3] = (16, 32 * G, nodes[3][2], 1, 0)                  # n3: 64 GiB -> 32 GiB
        lower = vc.make_cluster(nodes, vc.HAND_PARTS)
        code2, elig2 = ref.check(lower, jobs, ref.resv_node_sets(resv))
        assert not (np.array_equal(code2, want_code) and np.array_equal(elig2, want_elig)), "the lowered memory changes an answer"
        eng.set_nodes(lower)
        eng.set_reservations(resv)
        _same("after", eng.validate_jobs(jobs), code2, elig2)
    finally:
        eng.close()


def test_partitions_the_cycle_refuses(engine_default):
    """65 distinct res_total records in one partition (the cycle refuses it: CNS_PART_REFUSED_TYPES) are validated exactly; a partition
    with an unsupported node gives REFUSED for its own jobs only."""
    nodes = [(4, 8 * G, 0, 1, 0)] * 3 + [(8, (16 + i) * G, 0, 1, 0) for i in range(65)] + [(4, 8 * G, 0, 1, 1), (4, 8 * G, 0, 1, 0), (4, 8 * G, 0, 1, 0)]
    parts = [[0, 1, 2], list(range(3, 68)), [68, 69], [69, 70]]   # (partition 3 shares node 69 with the refused partition 2)
    cl = vc.make_cluster(nodes, parts)
    rows = [dict(p=1, tcpu=8 * CORE, tmem=(16 + i) * G) for i in range(0, 65, 4)]                # 65 - i nodes each
    rows += [dict(p=1, tcpu=CORE, tmem=40 * G, k=41, nt=41), dict(p=1, tcpu=CORE, tmem=40 * G, k=42, nt=42)]
    rows += [dict(p=2, tcpu=CORE, tmem=G), dict(p=3, tcpu=CORE, tmem=G), dict(p=0, tcpu=CORE, tmem=G)]
    jobs = vc.make_jobs(rows)
    want_code, want_elig = ref.check(cl, jobs, None)
    assert want_elig[:17].tolist() == [65 - i for i in range(0, 65, 4)] and want_code[17:19].tolist() == [abi.VALID_OK, abi.VALID_NOT_ENOUGH_NODES]
    assert want_code[19:].tolist() == [abi.VALID_REFUSED, abi.VALID_OK, abi.VALID_OK] and want_elig[20] == 2
    eng = _engine(engine_default, cl)
    try:
        status = eng.partition_status()
        assert int(status[1]) == 3 and int(status[0]) == 0          # CNS_PART_REFUSED_TYPES, CNS_PART_SERVED
        _same("refused by the cycle", eng.validate_jobs(jobs), want_code, want_elig)
    finally:
        eng.close()
