"""Giant partitions: one partition of up to 262 144 nodes that shares none, and one group of partitions that share nodes of up to
524 288 (partition, node) slots (an "ALL" partition over 262 144 nodes next to subsets that cover it once more).  Until now the
engine refused both (CNS_PART_REFUSED_WIDTH above 65 536 / 143 360 slots).  They run on k_giant: k_wide's home workgroup with the
sequential protocol, plus helper workgroups that scan stripes of the job's slots and answer round 0 of the walk; k_mem (the home
alone, 19-word row masks above 143 360 slots) is its exact fallback and is checked too (CNS_SELECT_KERNEL=mem).

Every case is checked against the CPU oracle on a prefix of C4's queue: placements, fp64 costs as bit patterns, the time maps of a
node sample, run-to-run determinism and the replay conservation check.  Routing of what fits the ordinary kernels does not change:
a giant partition beside ordinary ones leaves those on k_wide."""
import copy

import numpy as np
import pytest

from cranesched_amd import abi, synth
from oracle import pyoracle
from tests import helpers
from tests.test_gpu_fullsize import crc, replay_ok

pytestmark = pytest.mark.gpu

J_PART = 6000    # jobs of the single-partition cases (the oracle takes well under a second at these widths)
J_GROUP = 4000   # ... of the group cases (every decision of k_mem scans the job's partition: ~k_mem's cost per slot x 2 N)
MEM_SLOTS = 143_360   # what k_mem's ordinary row masks hold (wide_kernel.inc, kWMemWords): wider runs on its giant instantiation


def _cluster(c, parts):
    """c with its partitions replaced by `parts` (lists of node indices)."""
    off = np.cumsum([0] + [len(p) for p in parts]).astype(np.uint32)
    return abi.Cluster(c.cpu_total_raw, c.mem_total, c.core_lo, c.core_hi, c.gres_slots, off,
                       np.concatenate(parts).astype(np.uint32), gres=c.gres, schedulable=c.schedulable)


def _replay_ok(c, j, pl):
    """test_gpu_fullsize.replay_ok (no node over-subscribed when every placement is replayed) for any partition layout: membership is
    checked here against the partition's node list, the replay sees one partition over all nodes."""
    k = j.node_num.astype(np.int64)
    job_of = np.repeat(np.arange(j.num_jobs), k)
    node = got_nodes = pl.node_idx[:len(job_of)].astype(np.int64)
    live = got_nodes != abi.NODE_NONE
    po = c.part_offsets.astype(np.int64)
    for p in range(c.num_partitions):
        sel = live & (j.partition[job_of] == p)
        assert np.isin(node[sel], c.part_nodes[po[p]:po[p + 1]]).all(), f"node outside partition {p}"
    c1, j1 = copy.copy(c), copy.copy(j)
    c1.part_offsets = np.array([0, c.num_nodes], np.uint32)
    j1.partition = np.zeros(j.num_jobs, np.uint32)
    return replay_ok(c1, j1, pl)


def _run_and_check(eng_cls, c, j, now, tag, widest, running=None, reservations=None, sample_nodes=256):
    """widest: slots of the widest partition / group of the snapshot (k_mem's giant masks above MEM_SLOTS: the fallback runs)"""
    ref = pyoracle.select(c, j, now, running=running, reservations=reservations)
    eng = eng_cls(device=0)
    try:
        eng.set_nodes(c)
        if reservations is not None:
            eng.set_reservations(reservations)
        if running is not None:
            eng.set_running(running)
        got = eng.node_select(now, j)
        t = eng.timing()["select_ms"]
        k = eng.last_kernel()
        assert "k_giant" in k and "helper workgroups" in k, (tag, k)
        assert not eng.partition_status().any(), (tag, eng.partition_status())
        helpers.assert_same(eng, got, ref, c, sample_nodes=sample_nodes, tag=tag)
        c1 = crc(got)
        again = eng.node_select(now, j)
        assert crc(again) == c1, f"{tag}: run-to-run nondeterminism"
        if reservations is None and running is None:
            assert _replay_ok(c, j, got)
        print(f"{tag}: {j.num_jobs} jobs, {int(c.part_offsets[-1])} slots: {k} {t:.1f} ms = {1e3 * t / j.num_jobs:.1f} us per decision")
        return got, ref, k
    finally:
        eng.close()


@pytest.mark.parametrize("N", [131_072, 262_144])
def test_one_giant_partition(engine_default, N):
    """Case 1: ONE partition of 131 072 / 262 144 nodes (wider than k_wide's 65 536-slot tile) on a C4-style queue prefix."""
    c, j, now = synth.make_config("C4", J=J_PART, N=N, P=1)
    _run_and_check(engine_default, c, j, now, f"one partition of {N} nodes", N)


@pytest.mark.parametrize("N", [131_072, 262_144])
def test_all_partition_over_a_giant_cluster(engine_default, N):
    """Case 2: C4's partitions plus an ALL partition over every node: one group of 2 N = 262 144 / 524 288 slots (k_mem's ordinary masks
    hold 143 360)."""
    c, j, now = synth.make_mixed("C4all64k", J=J_GROUP, N=N)[:3]
    assert int(c.part_offsets[-1]) == 2 * N
    _run_and_check(engine_default, c, j, now, f"ALL over {N} nodes", 2 * N)


def test_giant_partition_with_running_jobs(engine_default):
    """Case 3a: running jobs folded into a 131 072-node partition (time maps with releases, partly used fronts)."""
    c, j, now = synth.make_config("C4", J=J_PART, N=131_072, P=1)
    run = synth.make_running(c, 20_000, seed=7, now=now)
    _run_and_check(engine_default, c, j, now, "one partition of 131 072 nodes + running", 131_072, running=run)


def _reservations(c, now, spans):
    """One reservation per (first node, count, start, end): every reserved node whole (its whole res_total)."""
    start, end, off, node = [], [], [0], []
    for first, cnt, s, e in spans:
        nd = np.arange(first, first + cnt, dtype=np.int64)
        node.append(nd); off.append(off[-1] + cnt); start.append(s); end.append(e)
    node = np.concatenate(node)
    return abi.Reservations(start, end, off, node, c.cpu_total_raw[node], c.mem_total[node], c.core_lo[node],
                            c.core_hi[node], c.gres_slots[node])


def test_giant_group_with_a_giant_reservation(engine_default):
    """Case 3b: ALL over 131 072 nodes + C4's subsets (a group of 262 144 slots) with an active reservation over 70 000 nodes — its virtual
    partition is wider than k_wide's tile and runs on k_mem too, inside a snapshot with shared nodes (the reservation's own slot range) —
    and a future one over 512 nodes (dips in the group's slots).  Every eleventh job asks for the active reservation."""
    N = 131_072
    c, j, now = synth.make_mixed("C4all64k", J=J_GROUP, N=N)[:3]
    rv = _reservations(c, now, [(1000, 70_000, now - 1000, now + 8 * 3600), (90_000, 512, now + 3600, now + 3 * 3600)])
    resv = np.full(j.num_jobs, abi.RESV_NONE, np.uint32)
    resv[np.arange(j.num_jobs) % 11 == 5] = 0
    j.reservation = resv
    _run_and_check(engine_default, c, j, now, "ALL over 131 072 nodes + reservations", 2 * N, reservations=rv)


def test_giant_partition_beside_ordinary_ones(engine_default):
    """Case 4: one cycle over a 131 072-node partition and four ordinary ones of 8 192 nodes: the ordinary ones stay on k_wide, the giant
    one runs on k_mem beside them, all of them against the oracle."""
    N_big, N_small, P_small = 131_072, 8192, 4
    c, j, now = synth.make_config("C4", J=J_PART, N=N_big + P_small * N_small, P=1)
    parts = [np.arange(N_big)] + [N_big + np.arange(N_small) + s * N_small for s in range(P_small)]
    c = _cluster(c, parts)
    j.partition = (np.arange(j.num_jobs) % (1 + P_small)).astype(np.uint32)
    _, _, k = _run_and_check(engine_default, c, j, now, "giant + ordinary partitions", N_big)
    assert k.startswith("k_wide"), k


def _edge(engine_default, parts, extra_nodes, refused, tag):
    """A snapshot whose first group sits at / just above the limit, next to a disjoint 1 000-node partition: the jobs of a refused group come
    back with REASON_ENGINE_REFUSED and nothing decided, the rest is bit-exact against the oracle on the queue without them."""
    N = extra_nodes + 1000
    c, j, now = synth.make_config("C4", J=3000, N=N, P=1)
    c = _cluster(c, parts + [np.arange(extra_nodes, N)])
    P = c.num_partitions
    j.partition = (np.arange(j.num_jobs) % P).astype(np.uint32)
    eng = engine_default(device=0)
    try:
        eng.set_nodes(c)
        got = eng.node_select(now, j)
        st = eng.partition_status()
        want = np.zeros(P, np.int64)
        want[refused] = abi.PART_REFUSED_WIDTH
        assert np.array_equal(st.astype(np.int64), want), (tag, st)
        ref_mask = np.isin(j.partition, np.asarray(refused, np.uint32))
        assert (got.reason[ref_mask] == abi.REASON_ENGINE_REFUSED).all() and (got.start_sec[ref_mask] == 0).all(), tag
        off = got.place_offsets
        for x in np.nonzero(ref_mask)[0]:
            assert (got.node_idx[off[x]:off[x + 1]] == abi.NODE_NONE).all(), tag
        served = [p for p in range(P) if p not in refused]
        sub, keep = synth.select_partitions(c, j, served)
        ref = pyoracle.select(c, sub, now)
        assert (got.reason[keep] == ref.placements.reason).all(), tag
        assert (got.start_sec[keep] == ref.placements.start_sec).all(), tag
        ro = ref.placements.place_offsets
        for x, jj in enumerate(keep):
            a, b = slice(off[jj], off[jj + 1]), slice(ro[x], ro[x + 1])
            for f in ("node_idx", "ntasks", "cpu_raw", "mem", "core_lo", "core_hi", "gres"):
                assert np.array_equal(getattr(got, f)[a], getattr(ref.placements, f)[b]), (tag, jj, f)
        print(f"{tag}: {eng.last_kernel()}")
    finally:
        eng.close()


def test_edge_one_partition_at_the_limit_is_served(engine_default):
    """Case 5a: 262 144 nodes in one partition are served."""
    _edge(engine_default, [np.arange(262_144)], 262_144, [], "262 144 nodes")


def test_edge_one_partition_above_the_limit_is_refused_alone(engine_default):
    """Case 5b: 262 145 nodes give CNS_PART_REFUSED_WIDTH for that partition only; the disjoint one beside it is served."""
    _edge(engine_default, [np.arange(262_145)], 262_145, [0], "262 145 nodes")


def test_edge_group_above_the_limit_is_refused_alone(engine_default):
    """Case 5c: a group of 524 289 slots (two partitions over 262 145 and 262 144 nodes that share them) is refused as a whole; the disjoint
    partition beside it is served.  (524 288 slots: ALL over 262 144 nodes, case 2.)"""
    _edge(engine_default, [np.arange(262_145), np.arange(262_144)], 262_145, [0, 1], "group of 524 289 slots")


@pytest.mark.parametrize("N,group", [(262_144, False), (131_072, True)])
def test_k_mem_fallback_on_giant_shapes(engine_default, monkeypatch, N, group):
    """CNS_SELECT_KERNEL=mem: the same shapes on k_mem alone (the fallback when the helpers' co-residency cannot be proven, and the retry
    after a protocol fault) — 19-word masks above 143 360 slots — bit-exact too, and the same result as k_giant's."""
    monkeypatch.setenv("CNS_SELECT_KERNEL", "mem")
    if group:
        c, j, now = synth.make_mixed("C4all64k", J=2000, N=N)[:3]
    else:
        c, j, now = synth.make_config("C4", J=2000, N=N, P=1)
    ref = pyoracle.select(c, j, now)
    eng = engine_default(device=0)
    try:
        eng.set_nodes(c)
        got = eng.node_select(now, j)
        k = eng.last_kernel()
        assert k.startswith("k_mem") and "k_giant" not in k and ("k_mem giant" in k) == (int(c.part_offsets[-1]) > MEM_SLOTS), k
        helpers.assert_same(eng, got, ref, c, sample_nodes=64, tag=f"k_mem {N}")
    finally:
        eng.close()


@pytest.mark.parametrize("seed,N,P", [(31, 40_000, 1), (32, 20_000, 2)])
def test_k_giant_forced_on_heterogeneous_queues(engine_default, monkeypatch, seed, N, P):
    """CNS_SELECT_KERNEL=giant on shapes k_wide would take: exclusive jobs, ntasks > node_num, include / exclude lists, multi-node jobs and
    running jobs — the walk past round 0 (the home's masks built on demand) and the jobs the home scans alone — against the oracle."""
    monkeypatch.setenv("CNS_SELECT_KERNEL", "giant")
    c, j, now, run = helpers.random_case(seed, N=N, J=2500, P=P, running=3000)
    eng = engine_default(device=0)
    try:
        eng.set_nodes(c)
        eng.set_running(run)
        got = eng.node_select(now, j)
        k = eng.last_kernel()
        assert k.startswith("k_giant"), k
        ref = pyoracle.select(c, j, now, running=run)
        helpers.assert_same(eng, got, ref, c, sample_nodes=64, tag=f"k_giant forced {seed}")
        assert crc(eng.node_select(now, j)) == crc(got)
    finally:
        eng.close()


def test_k_giant_forced_on_a_group_in_k_mem_s_range(engine_default, monkeypatch):
    """CNS_SELECT_KERNEL=giant on c4all64k (131 072 slots, k_mem by default): the helpers under shared nodes and own-partition ranges."""
    monkeypatch.setenv("CNS_SELECT_KERNEL", "giant")
    c, j, now = synth.make_mixed("C4all64k", J=J_GROUP)[:3]
    _run_and_check(engine_default, c, j, now, "c4all64k on k_giant", int(c.part_offsets[-1]))
