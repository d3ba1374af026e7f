"""Cases of the commit loop's checks (include/crane_gpu_commit/commit_check.h): a hand-made cycle and a seeded generator.
Shared by tests/test_commit_pyref.py (CPU: the generator is held to its coverage condition on the ORACLE's placements) and
tests/test_gpu_commit_check.py (the engine's cycle and call against tests/commit_pyref.py)."""
from __future__ import annotations

import functools

import numpy as np

from cranesched_amd import abi
from tests import kat
from tests.test_reservations import _resv

NOW = kat.NOW
NONE = abi.RESV_NONE
PAST = abi.CC_TIME_INFINITE_PAST
PENDING = abi.PREEMPT_REF_PENDING


def make_jobs(rows) -> abi.Jobs:
    """rows: dicts for kat.jobs, plus rsv (reservation index)."""
    j = kat.jobs(rows)
    j.reservation = np.asarray([r.get("rsv", NONE) for r in rows], np.uint32)
    return j


# ---- the hand-made cycle ---------------------------------------------------------------------------------------------------------------
# 8 nodes of 4 cores / 16 GiB.  p0 = {n0..n3}, p1 = {n4..n7}.  Reservations, all active at NOW and each taking its nodes whole:
#   r0 = {n4 n5} until NOW+5000      r1 = {n6} until NOW+150      r2 = {n7} until NOW+5000
# The events of the call: every node of p0 at NOW+100, n0..n3 again at NOW+400 (a later time never replaces, :1480-1481), n4..n7 at
# InfinitePast (reservation jobs do not look at node events, :1512-1521); affected reservations: r0 exists, ends NOW+5000, now = {n4};
# r1 exists, ends NOW+99; r2 is deleted.  The codes below hold WHEREVER the cycle puts the one-node jobs of p0 (every node of p0 has
# the same change time); job 7 is the one whose code depends on its node (n4: OK, n5: RESV_CHANGED) — the truth is the restatement fed
# with the cycle's own placements, and the GPU test asserts the rows marked sure.
HAND_ROWS = [
    # (job, gone, preempted list, code or None where it depends on the placement)
    (dict(part=0, L=100), 0, [], abi.COMMIT_OK),                                        # 0: change == end keeps the job
    (dict(part=0, L=101), 0, [], abi.COMMIT_RESOURCE_CHANGED),                          # 1: change == end - 1
    (dict(part=0, L=50, k=2), 0, [0], abi.COMMIT_WAITING_PREEMPTION),                   # 2: OK so far, its victim (running 0) is alive
    (dict(part=0, L=500), 1, [], abi.COMMIT_GONE),                                      # 3: gone comes first
    (dict(part=0, L=3000), 0, [0], abi.COMMIT_RESOURCE_CHANGED),                        # 4: ... before the preemption check
    (dict(part=0, L=60), 0, [PENDING | 0, 1], abi.COMMIT_OK),                           # 5: a pending reference to index 0, a dead victim
    (dict(part=0, L=100, cpu=4, k=4), 0, [], abi.COMMIT_NOT_STARTED),                   # 6: four whole nodes are not free: a reason
    (dict(part=1, L=100, rsv=0), 0, [], None),                                          # 7: n4 or n5
    (dict(part=1, L=100, rsv=0, k=2), 0, [], abi.COMMIT_RESV_CHANGED),                  # 8: n4 and n5: n5 left the reservation
    (dict(part=1, L=100, rsv=1), 0, [], abi.COMMIT_RESV_ENDS_EARLY),                    # 9: NOW+99 < NOW+100
    (dict(part=1, L=99, rsv=1), 0, [], abi.COMMIT_OK),                                  # 10: NOW+99 == end; n6 is still listed
    (dict(part=1, L=100, rsv=2), 0, [], abi.COMMIT_RESV_DELETED),                       # 11
    (dict(part=1, L=100, rsv=2, cpu=4), 0, [], abi.COMMIT_NOT_STARTED),                 # 12: n7 has 3 cores left: backfilled, a reason
]


def hand():
    """-> (cluster, reservations, jobs, now, events, commit jobs, sure codes [(job, code)])"""
    cl = kat.cluster([4] * 8, parts=[[0, 1, 2, 3], [4, 5, 6, 7]])
    whole = lambda n: (n, 4, 16, 0xF)
    rv = _resv([(NOW - 10, NOW + 5000, [whole(4), whole(5)]), (NOW - 10, NOW + 150, [whole(6)]), (NOW - 10, NOW + 5000, [whole(7)])])
    jobs = make_jobs([r[0] for r in HAND_ROWS])
    ev = abi.CommitEvents(node_events=[(NOW + 100, [0, 1, 2, 3]), (NOW + 400, [3, 2, 1, 0]), (PAST, [4, 5, 6, 7])],
                          affected_resv=[(2, 0, 0, []), (0, 1, NOW + 5000, [4]), (1, 1, NOW + 99, [6])])
    off, flat = abi._csr([r[2] for r in HAND_ROWS])
    cj = abi.CommitJobs(time_limit_sec=jobs.time_limit_sec, reservation=jobs.reservation, gone=[r[1] for r in HAND_ROWS],
                        preempt_offsets=off, preempted=flat, running_alive=[1, 0])
    return cl, rv, jobs, NOW, ev, cj, [(j, r[3]) for j, r in enumerate(HAND_ROWS) if r[3] is not None]


# ---- the generator ---------------------------------------------------------------------------------------------------------------------
SEEDS = (0, 1, 2, 3, 4, 5)
NUM_RUNNING = 16      # the running table the generated preempted lists point into


def generate(seed: int):
    """A seeded cluster (<= 300 nodes of 8 cores in 2 - 4 disjoint partitions, 2 active reservations that take their nodes whole) and
    <= 2 000 jobs, 90 % of them one-node jobs, the others 2 - 130 nodes wide, a sixth of them into the reservations.
    -> (cluster, reservations, jobs, now)"""
    rng = np.random.default_rng(7000 + seed)
    P = int(rng.integers(2, 5))
    big = int(rng.integers(150, 200))                                  # partition 0 holds the wide jobs
    sizes = [big] + [int(rng.integers(10, max(11, (300 - big) // (P - 1)))) for _ in range(P - 1)]
    N = sum(sizes)
    bounds = np.concatenate([[0], np.cumsum(sizes)])
    parts = [list(range(int(bounds[p]), int(bounds[p + 1]))) for p in range(P)]
    cl = kat.cluster([8] * N, mem_gib=[64] * N, parts=parts)
    # reservation 0: the last 66 - 80 nodes of partition 0 (wide enough for a 65-node job, and 130 nodes stay outside it); reservation 1:
    # 3 - 6 nodes of partition 1
    r0 = parts[0][-int(rng.integers(66, 81)):]
    r1 = parts[1][:int(rng.integers(3, 7))]
    whole = lambda n: (n, 8, 64, 0xFF)
    rv = _resv([(NOW - 100, NOW + 20000, [whole(n) for n in r0]), (NOW - 100, NOW + 20000, [whole(n) for n in r1])])
    J = int(rng.integers(600, 2001))
    rows = []
    for _ in range(J):
        r = dict(part=int(rng.integers(0, P)), cpu=int(rng.choice([1, 2, 4])), L=int(rng.choice([60, 100, 300, 900, 3600])))
        u = rng.random()
        if u < 0.10:
            r["part"] = 0
            r["k"] = int(rng.choice([2, 3, 7, 8, 9, 33, 64, 65, 130]))
            if r["k"] > 60 and rng.random() < 0.5:
                r["L"] = 60
        v = rng.random()
        if v < 0.12:
            r.update(part=0, rsv=0)
            if "k" in r:
                r["k"] = min(r["k"], 65)
        elif v < 0.17:
            r.update(part=1, rsv=1)
            r["k"] = int(rng.choice([1, 1, 2, 3]))
        rows.append(r)
    return cl, rv, make_jobs(rows), NOW


def draw_call(seed: int, jobs: abi.Jobs, pl: abi.Placements, rv: abi.Reservations):
    """The events and job arrays of a call, drawn from a cycle's placements `pl`: node events on nodes that started jobs use, with times
    on either side of their ends; reservation 0 and reservation 1 affected in a way that turns with the seed (deleted / ends inside its
    jobs' ends / lost some of the nodes its jobs were placed on); 3 % of the jobs gone; preempted lists (made up: the cycle of the
    generator runs without preemption, and the call takes the lists as input) on 5 % of the jobs, into a running table of NUM_RUNNING
    jobs of which half are alive.  -> (abi.CommitEvents, abi.CommitJobs)"""
    rng = np.random.default_rng(9000 + seed)
    J = jobs.num_jobs
    started = np.flatnonzero(pl.reason[:J] == 0)
    end = pl.start_sec[:J] + jobs.time_limit_sec
    rec = lambda j: [int(n) for n in pl.node_idx[int(pl.place_offsets[j]):int(pl.place_offsets[j + 1])] if n != abi.NODE_NONE]
    plain = [int(j) for j in started if jobs.reservation[j] == NONE]
    node_events = []
    for j in rng.choice(plain, min(len(plain), 14), replace=False).tolist() if plain else []:
        t = int(end[j]) + int(rng.choice([-1, 0, 1, 1, 500]))
        nodes = [int(rng.choice(rec(j)))]
        for o in rng.choice(plain, 3).tolist():                       # ... and nodes of other started jobs, whatever their ends
            nodes.append(int(rng.choice(rec(o))))
        node_events.append((t, nodes))
    if plain and seed % 2 == 0:
        node_events.append((PAST, rec(plain[0])[:1]))
    # a wide job's last record
    widest = max(plain, key=lambda j: len(rec(j)), default=None)
    if widest is not None and len(rec(widest)) > 1:
        node_events.append((int(end[widest]) - 1, rec(widest)[-1:]))
    node_events.append((NOW + 7, []))                                 # an event without nodes
    affected = []
    for v in (0, 1):
        mine = [int(j) for j in started if jobs.reservation[j] == v]
        lo, hi = int(rv.alloc_offsets[v]), int(rv.alloc_offsets[v + 1])
        listed = [int(n) for n in rv.alloc_node[lo:hi]]
        mode = (seed + 2 * v) % 3
        if not mine or mode == 0:
            affected.append((v, 0, 0, []))                            # deleted
            continue
        ends = sorted(int(end[j]) for j in mine)
        used = sorted({n for j in mine for n in rec(j)})
        if mode == 1:                                                 # ends where half of its jobs' ends lie behind it; the node list is whole
            affected.append((v, 1, ends[len(ends) // 2], listed[::-1]))
        else:                                                         # still long enough; every third used node left it
            affected.append((v, 1, ends[-1], [n for n in listed if n not in used[::3]]))
    gone = (rng.random(J) < 0.03).astype(np.uint8)
    lists = [[] for _ in range(J)]
    alive = (np.arange(NUM_RUNNING) % 2).astype(np.uint8)
    for j in rng.choice(J, max(1, J // 20), replace=False).tolist():
        n = int(rng.integers(1, 4))
        lists[j] = [int(rng.integers(0, NUM_RUNNING)) if rng.random() < 0.7 else PENDING | int(rng.integers(0, J)) for _ in range(n)]
    off, flat = abi._csr(lists)
    order = rng.permutation(len(affected))
    ev = abi.CommitEvents(node_events=node_events, affected_resv=[affected[i] for i in order])
    cj = abi.CommitJobs(time_limit_sec=jobs.time_limit_sec, reservation=jobs.reservation, gone=gone, preempt_offsets=off, preempted=flat,
                        running_alive=alive)
    return ev, cj


@functools.lru_cache(maxsize=None)
def generated(seed: int):
    """generate(seed), the ORACLE's cycle over it, the call drawn from that cycle's placements and the truth's answer; computed once per
    process.  -> (cluster, reservations, jobs, now, oracle placements, events, commit jobs, code, counts)"""
    from oracle import pyoracle
    from tests import commit_pyref
    cl, rv, jobs, now = generate(seed)
    run = pyoracle.select(cl, jobs, now, reservations=rv)
    pl = run.placements
    ev, cj = draw_call(seed, jobs, pl, rv)
    code, counts = commit_pyref.check(pl.start_sec, pl.reason, pl.place_offsets, pl.node_idx, ev, cj)
    return cl, rv, jobs, now, pl, ev, cj, code, counts


def widths(jobs: abi.Jobs, pl: abi.Placements) -> np.ndarray:
    """placement records of every job that name a node"""
    J = jobs.num_jobs
    named = np.concatenate([[0], np.cumsum(pl.node_idx[:int(pl.place_offsets[J])] != abi.NODE_NONE)])
    return (named[pl.place_offsets[1:J + 1].astype(np.int64)] - named[pl.place_offsets[:J].astype(np.int64)]).astype(np.int64)
