"""Random clusters and queries for the reservation what-ifs (include/crane_gpu_resv/resv_probe.h), shared by tests/test_gpu_resvq.py.

A cluster: 1..300 nodes, some unschedulable, some in no partition; 0..3 reservations per node (overlapping ones too, expired ones,
one that never ends) and 0..8 running allocations per node, some of jobs that run inside a reservation, some on unschedulable nodes.
Every end is drawn from 8 distinct times (+ "never"), so the event times of an earliest-start search hold many equal values.
Queries: lists of the lengths that cross the wave / workgroup / chunk edges of the pick kernel, with the free nodes pushed to both
ends of the list, k at 0, 1, num_free and num_free + 1, both modes, a few in the past, a few candidates that do not exist."""
from __future__ import annotations

import numpy as np

from cranesched_amd import abi
from tests import resvq_pyref as ref

NOW = 1_000_000
INF = ref.INT64_MAX
LIST_LENGTHS = (1, 63, 64, 65, 511, 512, 513, 1025)
SEEDS = (0, 1, 2, 3)
G = 1 << 30


def random_cluster(seed: int, N: int | None = None):
    """-> (cluster, running, reservations, times): the 8 distinct times the ends are drawn from."""
    rng = np.random.default_rng(0x5E5F + seed)
    if N is None:
        N = int(rng.integers(1, 301))
    times = np.sort(rng.choice(np.arange(-4, 40), 8, replace=False)) * 600 + NOW
    sched = (rng.random(N) < 0.85).astype(np.uint8)
    in_part = rng.random(N) < 0.9                        # the others are in no partition
    members = np.flatnonzero(in_part).astype(np.uint32)
    if len(members) == 0:
        members = np.array([0], np.uint32)
    half = len(members) // 2
    cluster = abi.Cluster(np.full(N, 8 * 256, np.int64), np.full(N, 32 * G, np.uint64), np.full(N, 0xFF, np.uint64), np.zeros(N, np.uint64),
                          np.zeros(N, np.uint64), np.array([0, half, len(members)], np.uint32), members, schedulable=sched)
    # reservations: V of them over random node sets, so that a node is listed by 0..3
    per_node = rng.choice([0, 0, 0, 1, 1, 2, 3], N)
    V = 12
    rv_nodes = [[] for _ in range(V)]
    for n in range(N):
        for v in rng.choice(V, per_node[n], replace=False):
            rv_nodes[int(v)].append(n)
    rs, re = np.zeros(V, np.int64), np.zeros(V, np.int64)
    for v in range(V):
        a, b = sorted(rng.choice(8, 2, replace=False))
        rs[v], re[v] = times[a] + int(rng.integers(-1, 2)), times[b]   # starts one second off the grid too: the st == start + duration edge
    re[V - 1] = INF                                      # one reservation never ends
    roff = np.concatenate([[0], np.cumsum([len(x) for x in rv_nodes])]).astype(np.uint32)
    rnode = np.array([n for x in rv_nodes for n in x], np.uint32)
    m = len(rnode)
    resv = abi.Reservations(rs, re, roff, rnode, np.full(m, 256, np.int64), np.full(m, G, np.uint64), np.ones(m, np.uint64),
                            np.zeros(m, np.uint64), np.zeros(m, np.uint64))
    # running jobs: 0..8 allocations per node (most nodes: none), one- and two-node jobs, a tenth of them inside a reservation
    per_node = np.where(rng.random(N) < 0.5, 0, rng.integers(0, 9, N))
    ends, offs, nodes, rsv = [], [0], [], []
    for n in range(N):
        for _ in range(int(per_node[n])):
            e = INF if rng.random() < 0.03 else int(times[rng.integers(0, 8)])
            alloc = [n] if rng.random() < 0.7 or N == 1 else sorted({n, int(rng.integers(0, N))})
            ends.append(e)
            nodes += alloc
            offs.append(len(nodes))
            rsv.append(int(rng.integers(0, V)) if rng.random() < 0.1 else abi.RESV_NONE)
    m = len(nodes)
    running = abi.Running(np.array(ends, np.int64), np.array(offs, np.uint32), np.array(nodes, np.uint32), np.full(m, 256, np.int64),
                          np.full(m, G, np.uint64), np.ones(m, np.uint64), np.zeros(m, np.uint64), np.zeros(m, np.uint64),
                          reservation=np.array(rsv, np.uint32))
    return cluster, running, resv, times


def random_queries(seed: int, N: int, state: ref.NodeState, times, Q: int, lengths=LIST_LENGTHS):
    """Q queries over a cluster of N nodes; query i has list length lengths[i % len(lengths)] (lists longer than the cluster are
    filled with node indices that do not exist)."""
    rng = np.random.default_rng(0xC0FE + seed)
    starts, durs, ks, mode, off, cand = [], [], [], [], [0], []
    for i in range(Q):
        L = lengths[i % len(lengths)]
        start = int(times[rng.integers(0, 6)]) + int(rng.integers(-1, 2))
        dur = int(rng.choice([1, 600, 601, 1800, 7200]))
        real = rng.permutation(N)[:min(N, L)]
        ghosts = N + rng.permutation(4 * L)[:L - len(real)]          # "not found", distinct
        lst = np.concatenate([real, ghosts]).astype(np.int64)
        # the free nodes (at the start) to both ends of the list, the others in between
        _, _, codes, _ = ref.at_start(state, start, dur, 0, [int(x) for x in lst])
        free = lst[np.array(codes) == ref.FREE]
        busy = rng.permutation(lst[np.array(codes) != ref.FREE])
        lst = np.concatenate([free[:len(free) // 2], busy, free[len(free) // 2:]]) if i % 3 else rng.permutation(lst)
        nf = len(free)
        k = [0, 1, nf, nf + 1][int(rng.integers(0, 4))]
        if i % 11 == 10:                                            # in the past
            start, dur = NOW - 5000, int(rng.choice([1, 5000]))
        starts.append(start); durs.append(dur); ks.append(k); mode.append(int(rng.random() < 0.5))
        cand += [int(x) for x in lst]
        off.append(len(cand))
    return abi.ResvQueries(np.array(starts, np.int64), np.array(durs, np.int64), np.array(ks, np.uint32), np.array(off, np.uint64),
                           np.array(cand, np.uint32), np.array(mode, np.uint8))


def same(tag: str, got: dict, exp: dict):
    for f in abi.ResvAnswers.FIELDS:
        g, e = np.asarray(got[f]), np.asarray(exp[f])
        assert g.shape == e.shape, f"{tag}: {f} has {g.shape} entries, expected {e.shape}"
        bad = np.flatnonzero(g != e)
        assert len(bad) == 0, f"{tag}: {f} differs at {bad[:8]} (got {g[bad[:8]]}, expected {e[bad[:8]]}), {len(bad)} in all"
