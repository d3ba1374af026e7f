"""Deterministic scenarios for the reservation what-ifs (include/crane_gpu_resv/resv_probe.h) that sit ON the seams of the device code
(csrc/resvq_kernels.inc, csrc/resvq_host.inc, the radix sort of csrc/sort_kernels.inc), where tests/resvq_case.py's random
scenarios never go: times over the whole signed 64-bit range, long chains of blocked ranges per node, empty lists and jobs without an
allocation, every number of radix passes over the segment numbers, a sort wider than one step of its scan, one handle across sizes.

Every generator returns a Seam (cluster, running, resv, queries, now).  The constants come from cns_resvq_shape (`shape`, an
abi.ResvqShape) and from csrc/sort_host.inc (the digit width), never from a literal here.  The truth stays resvq_pyref.answer:
expected() evaluates it once per DISTINCT query — queries are answered independently of one another — and replicates the answers.

Used by tests/test_resvq_seams.py (no GPU: do the generators hit what they name?) and tests/test_gpu_resvq_seams.py."""
from __future__ import annotations

import functools
import os
import re
from collections import namedtuple

import numpy as np

from cranesched_amd import abi
from tests import resvq_pyref as ref

INF = ref.INT64_MAX
INT64_MIN = -(1 << 63)
GRID = 600
NOW = 1_700_000_123            # (not the 1 000 000 of tests/resvq_case.py)
WIDE_NOW = -(1 << 62)
G = 1 << 30

Seam = namedtuple("Seam", ("cluster", "running", "resv", "queries", "now"))


def digit_bits() -> int:
    """The digit width of the sort's passes, from the file that defines it for every caller of the sort (csrc/sort_host.inc)."""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cranesched_amd", "csrc", "sort_host.inc")).read()
    return int(re.search(r"kDigitBits = (\d+);", src).group(1))


def last_q_of(passes: int) -> int:
    """The largest query count whose segment numbers 0 .. 2 Q - 1 fit in `passes` digits."""
    return (1 << (digit_bits() * passes)) // 2


def seg_passes(num_queries: int) -> int:
    p = 1
    while p < 4 and (2 * num_queries - 1) >> (digit_bits() * p):
        p += 1
    return p


# ---- building blocks ---------------------------------------------------------------------------------------------------------------
def _cluster(N: int):
    return abi.Cluster(np.full(N, 8 * 256, np.int64), np.full(N, 32 * G, np.uint64), np.full(N, 0xFF, np.uint64), np.zeros(N, np.uint64),
                       np.zeros(N, np.uint64), np.array([0, N], np.uint32), np.arange(N, dtype=np.uint32), schedulable=np.ones(N, np.uint8))


def _csr(lists):
    off = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    flat = np.array([v for x in lists for v in x], np.uint32)
    return off, flat


def _running(jobs):
    """jobs: [(end, [nodes])]; a job may have no allocation."""
    off, node = _csr([x for _, x in jobs])
    m = len(node)
    return abi.Running(np.array([e for e, _ in jobs], np.int64), off.astype(np.uint32), node, np.full(m, 256, np.int64), np.full(m, G, np.uint64),
                       np.ones(m, np.uint64), np.zeros(m, np.uint64), np.zeros(m, np.uint64))


def _resv(rows):
    """rows: [(start, end, [nodes])]."""
    off, node = _csr([x for _, _, x in rows])
    m = len(node)
    return abi.Reservations(np.array([s for s, _, _ in rows], np.int64), np.array([e for _, e, _ in rows], np.int64), off.astype(np.uint32), node,
                            np.full(m, 256, np.int64), np.full(m, G, np.uint64), np.ones(m, np.uint64), np.zeros(m, np.uint64), np.zeros(m, np.uint64))


def _queries(rows):
    """rows: [(start, duration, node_num, find_earliest, [candidates])]."""
    off, cand = _csr([r[4] for r in rows])
    return abi.ResvQueries(np.array([r[0] for r in rows], np.int64), np.array([r[1] for r in rows], np.int64), np.array([r[2] for r in rows], np.uint32),
                           off.astype(np.uint64), cand, np.array([r[3] for r in rows], np.uint8))


def state_of(seam: Seam) -> ref.NodeState:
    return ref.NodeState(seam.cluster.num_nodes, seam.running, seam.resv)


def _k_around_num_free(state, i, start, dur, cand):
    nf = ref.at_start(state, start, dur, 0, cand)[1]
    return (nf, nf + 1, 0, 1)[(i + i // 4) % 4]         # (every k with every mode, where the mode follows i % 4)


# ---- the reference, once per distinct query ------------------------------------------------------------------------------------------
def _gather_csr(doff, dval, inv):
    doff = np.asarray(doff).astype(np.int64)
    lens = np.diff(doff)[inv]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    idx = np.arange(int(off[-1]), dtype=np.int64) + np.repeat(doff[:-1][inv] - off[:-1], lens)
    return off, np.asarray(dval)[idx]


def distinct(q: abi.ResvQueries):
    """-> (rep, inv): query i equals query rep[inv[i]] in (start, duration, node_num, mode, list).  Grouped by a 64-bit hash, then
    VERIFIED field by field and candidate by candidate: a collision fails here, it never merges two different queries."""
    u64 = np.uint64
    off = q.cand_offsets.astype(np.int64)
    lens = np.diff(off)
    mode = np.zeros(q.num_queries, np.uint8) if q.find_earliest is None else q.find_earliest
    pos = (np.arange(len(q.cand_nodes), dtype=np.int64) - np.repeat(off[:-1], lens)).astype(u64)
    term = (q.cand_nodes.astype(u64) + u64(1)) * (pos * u64(0x9E3779B97F4A7C15) + u64(0xD1B54A32D192ED03))
    cs = np.concatenate([np.zeros(1, u64), np.cumsum(term, dtype=u64)])
    h = cs[off[1:]] - cs[off[:-1]]
    for col, mul in ((q.start_sec.view(u64), 0xFF51AFD7ED558CCD), (q.duration_sec.view(u64), 0xC4CEB9FE1A85EC53), (q.node_num.astype(u64), 0x2545F4914F6CDD1D),
                     (mode.astype(u64), 0x9FB21C651E98DF25), (lens.astype(u64), 0xA0761D6478BD642F)):
        h = (h ^ col) * u64(mul)
        h ^= h >> u64(29)
    _, rep, inv = np.unique(h, return_index=True, return_inverse=True)
    inv = inv.reshape(-1)
    for a in (q.start_sec, q.duration_sec, q.node_num, mode, lens):
        assert np.array_equal(a[rep][inv], a), "hash collision between two different queries"
    rep_off = np.concatenate([[0], np.cumsum(lens[rep])])
    rep_val = np.concatenate([q.cand_nodes[int(off[r]):int(off[r + 1])] for r in rep]) if len(rep) else np.zeros(0, np.uint32)
    assert np.array_equal(_gather_csr(rep_off, rep_val, inv)[1], q.cand_nodes), "hash collision between two different lists"
    return rep, inv


def expected(state: ref.NodeState, now: int, q: abi.ResvQueries) -> dict:
    """resvq_pyref.answer(state, now, q), computed once per distinct query."""
    rep, inv = distinct(q)
    d = q.take(rep)
    a = ref.answer(state, now, d)
    _, code = _gather_csr(d.cand_offsets, a["code"], inv)
    choff, chosen = _gather_csr(a["chosen_offsets"], a["chosen_nodes"], inv)
    return {"status": a["status"][inv], "start_sec": a["start_sec"][inv], "num_free": a["num_free"][inv], "code": code.astype(np.uint8),
            "chosen_offsets": choff.astype(np.uint64), "chosen_nodes": chosen.astype(np.uint32)}


# ---- wide_times ----------------------------------------------------------------------------------------------------------------------
BIG_DURATION = (1 << 62) + (1 << 61)      # st - (d - 1) leaves the range for every st below -2^61


def wide_times(shape) -> Seam:
    """now = -2^62; node ends, reservation bounds and query starts over the whole signed range (every byte of the sort key varies),
    both signs on both sides, ends at INT64_MIN + small, reservations from INT64_MIN, from and to INT64_MAX, durations 1 and one
    that saturates st - (d - 1).  Lists of at most 65 candidates and 60 queries: distinct times make the brute force quadratic."""
    rng = np.random.default_rng(0x51DE)
    N, now = 72, WIDE_NOW
    anchors = sorted({int(x) for x in rng.integers(INT64_MIN + (1 << 20), INF - (1 << 20), 22, dtype=np.int64)} | {-1, 0, 1, now, now + 1, -(1 << 61), 1 << 61})
    pick = lambda: anchors[int(rng.integers(0, len(anchors)))] + int(rng.integers(-1, 2))
    jobs = []
    for n in range(N):
        if n % 3 == 0:
            jobs.append((pick(), [n]))
        if n % 9 == 1:
            jobs.append((INT64_MIN + 1 + int(rng.integers(0, 50)), [n]))          # the fill of latest_end meets a very negative end
        if n % 12 == 6:
            jobs.append((pick(), sorted({n, (n * 5 + 1) % N})))
    jobs.append((INF, [5]))                                                       # never ends
    jobs.append((INT64_MIN, [8]))                                                 # equals the fill
    rows = []
    for n in range(N):
        for _ in range(n % 4):
            a, b = pick(), pick()
            if a != b:
                rows.append((min(a, b), max(a, b), [n]))
    rows += [(INT64_MIN, pick(), [10, 20]), (INT64_MIN, INT64_MIN + 40, [11]), (INF, INF, [12, 13]), (pick(), INF, [13, 21]), (INT64_MIN, INF, [14]),
             (-5, 5, [15, 16, 17]), (INF - 1, INF, [16])]
    cluster, running, resv = _cluster(N), _running(jobs), _resv(rows)
    state = ref.NodeState(N, running, resv)
    durs = (1, GRID, 1 << 40, BIG_DURATION, 1, INF)
    lengths = (1, 5, 33, shape.pick_block // 4, shape.pick_block // 4 + 1)
    qrows = []
    for i in range(60):
        d = durs[i % len(durs)]
        if i % 15 == 14:
            start = now - 1_000_000 - d if d < (1 << 50) else INT64_MIN + 9     # in the past (a huge duration from the far past is not)
        elif d >= BIG_DURATION:
            start = (INT64_MIN + 5, -(1 << 62) - 3, -7, INF - d)[(i // len(durs)) % 4]
        else:
            start = pick()
        start = min(start, INF - d)
        L = lengths[i % len(lengths)]
        cand = [int(x) for x in rng.permutation(N)[:L]]
        if i % 7 == 3:
            cand[len(cand) // 2] = N + i                                          # one that does not exist
        qrows.append((start, d, _k_around_num_free(state, i, start, d, cand), int(i % 4 != 1), cand))
    return Seam(cluster, running, resv, _queries(qrows), now)


# ---- dense_nodes ---------------------------------------------------------------------------------------------------------------------
DENSE_RESV_PER_NODE = 40
DENSE_INF_NODE = 7
MENU = ("disjoint", "overlapping", "nested", "twice", "off_grid")


def dense_nodes(shape) -> Seam:
    """130 nodes with 40 reservations each from a fixed menu on a 600 s grid: disjoint, overlapping, nested (the inner ones end with
    the outer one), identical twice, one second off the grid; between two blocks a gap of 0, 1 or 2 grid steps, so that for the
    durations 1, 600 and 601 a blocked range begins exactly where the last one ended (a == cur), one second later, or leaves a real gap.
    Starts on the grid meet reservations that end exactly there (ed == a).  Node 7 has an end at INT64_MAX in the middle of its list."""
    rng = np.random.default_rng(0xDE45E)
    N, now = 130, NOW
    base = (now // GRID + 1) * GRID
    rows, jobs = [], []
    for n in range(N):
        mine = []
        x = base + GRID * (int(rng.integers(0, 6)) - 8)                           # the first blocks lie before every start
        while len(mine) < DENSE_RESV_PER_NODE:
            kind = MENU[(n + len(mine) + int(rng.integers(0, 2))) % len(MENU)]
            if kind == "disjoint":
                mine.append((x, x + GRID)); x += GRID
            elif kind == "overlapping":
                mine += [(x, x + 2 * GRID), (x + GRID, x + 3 * GRID)]; x += 3 * GRID
            elif kind == "nested":
                mine += [(x, x + 4 * GRID), (x + GRID, x + 2 * GRID), (x + 2 * GRID, x + 4 * GRID)]; x += 4 * GRID
            elif kind == "twice":
                mine += [(x, x + GRID), (x, x + GRID)]; x += GRID
            else:
                mine.append((x + 1, x + GRID - 1)); x += GRID
            x += GRID * int(rng.choice([0, 1, 1, 2]))
        mine = mine[:DENSE_RESV_PER_NODE]
        if n == DENSE_INF_NODE:
            mine[DENSE_RESV_PER_NODE // 2] = (mine[DENSE_RESV_PER_NODE // 2][0], INF)
        rows += [(s, e, [n]) for s, e in mine]
        if n % 3 == 0:
            jobs.append((base + GRID * int(rng.integers(-2, 30)), [n]))
    order = rng.permutation(len(rows))                                            # the table's order is not the nodes' order
    rows = [rows[int(i)] for i in order]
    cluster, running, resv = _cluster(N), _running(jobs), _resv(rows)
    state = ref.NodeState(N, running, resv)
    L = shape.pick_block // 4 + 1
    qrows = []
    for i in range(64):
        d = (1, GRID, GRID + 1)[i % 3]
        start = base + GRID * int(rng.integers(0, 60)) + (0, 0, 1, -1)[(i // 3) % 4]
        cand = [int(x) for x in rng.permutation(N)[:L]]
        if i % 16 == 5 and DENSE_INF_NODE not in cand:
            cand[3] = DENSE_INF_NODE
        if i % 8 == 0:
            cand[L - 2] = N + 3
        nf = ref.at_start(state, start, d, 0, cand)[1]
        k = L if i % 21 == 20 else (nf, nf + 1)[(i // 4) % 2]
        qrows.append((start, d, k, int(i % 4 != 3), cand))
    return Seam(cluster, running, resv, _queries(qrows), now)


# ---- empties -------------------------------------------------------------------------------------------------------------------------
def _small_state():
    N, now = 12, NOW
    base = (now // GRID + 1) * GRID
    # jobs without an allocation: first, two adjacent in the middle, last
    jobs = [(base + 50 * GRID, []), (base + 2 * GRID, [0]), (base + 9 * GRID, []), (INF, []), (base + 4 * GRID, [1, 2]), (base + GRID, [3]), (base + 3 * GRID, [1]),
            (base + 70 * GRID, [])]
    rows = [(base, base + 3 * GRID, [2, 4]), (base + 5 * GRID, base + 6 * GRID, [4, 5, 6]), (base + GRID, INF, [7]), (base - 9 * GRID, base - GRID, [8])]
    return N, now, base, _cluster(N), _running(jobs), _resv(rows)


def empties(shape, variant: str = "lists") -> Seam:
    """"lists": 2 * pick_grid + 1 queries (a pick workgroup takes three), runs of three and four empty candidate lists at the front, in
    the middle and at the end with node_num 0 and 5, an earliest-start query whose candidates do not exist, running jobs without an
    allocation first, last and adjacent.  "all_past": every earliest-start query lies in the past (the call sorts nothing), the
    queries at a given start are live."""
    N, now, base, cluster, running, resv = _small_state()
    rng = np.random.default_rng(0xE3977)
    qrows = []
    if variant == "all_past":
        for i in range(9):
            cand = [int(x) for x in rng.permutation(N)[:1 + i % 5]]
            if i % 3 == 2:
                qrows.append((base + GRID * (i % 4), GRID, 1 + i % 2, 0, cand))
            else:
                qrows.append((now - 5000 - i, (1, 4000)[i % 2], 1, 1, cand))
        return Seam(cluster, running, resv, _queries(qrows), now)
    assert variant == "lists"
    Q = 2 * shape.pick_grid + 1
    mid = Q // 2
    empty = set(range(3)) | set(range(mid, mid + 4)) | set(range(Q - 3, Q))
    for i in range(Q):
        start = base + GRID * (i % 7) + (0, 1, -1)[i % 3]
        d = (1, GRID, GRID + 1, 4 * GRID)[i % 4]
        if i in empty:
            qrows.append((start, d, (0, 5)[i % 2], int(i % 3 != 0), []))
        elif i == 5:
            qrows.append((start, d, 2, 1, [N + 1, N + 5, N + 9]))                 # earliest, and nothing exists
        elif i == mid - 1:
            qrows.append((now - 9000, 100, 0, 1, []))                             # empty and in the past
        else:
            cand = [int(x) for x in rng.permutation(N)[:1 + i % 6]]
            qrows.append((start, d, (0, 1, 2)[i % 3], int(i % 5 != 0), cand))
    return Seam(cluster, running, resv, _queries(qrows), now)


# ---- three_passes / four_passes ------------------------------------------------------------------------------------------------------
def _one_candidate_each(cluster, running, resv, now, Q, distinct_rows):
    """Q queries tiled from `distinct_rows`, so that neighbours and queries 2^8, 2^16, 2^24 apart differ: a segment that lands in
    another one's place changes an answer."""
    d = _queries(distinct_rows)
    q = np.arange(Q, dtype=np.int64)
    inv = (q * 37 + (q >> 8) * 11 + (q >> 16) * 5 + (q >> 24) * 3) % len(distinct_rows)
    off = np.arange(Q + 1, dtype=np.uint64)
    return Seam(cluster, running, resv, abi.ResvQueries(d.start_sec[inv], d.duration_sec[inv], d.node_num[inv], off, d.cand_nodes[inv], d.find_earliest[inv]), now)


def three_passes(shape, Q: int | None = None) -> Seam:
    """last_q_of(2) + 1 earliest-start queries of one candidate each over 300 nodes with 0..2 reservations, starts over 7 values."""
    if Q is None:
        Q = last_q_of(2) + 1
    rng = np.random.default_rng(0x3FA55)
    N, now = 300, NOW
    base = (now // GRID + 1) * GRID
    times = [base + GRID * t for t in (0, 2, 3, 7, 12, 20, 31, 45)]
    jobs = [(times[int(rng.integers(0, 8))] if n % 17 else INF, [n]) for n in range(N) if n % 2]
    rows = []
    for v in range(30):
        a, b = sorted(int(x) for x in rng.choice(8, 2, replace=False))
        rows.append((times[a] + int(rng.integers(-1, 2)), times[b], [n for n in range(N) if (n * 7 + v) % 30 < 2]))
    rows.append((times[3], INF, [11, 12]))
    starts = [times[t] + j for t, j in ((0, 0), (0, 1), (1, -1), (2, 0), (4, 0), (5, 1), (6, 0))]
    drows = [(starts[(n + r) % 7], (1, GRID, GRID + 1)[(n // 7 + r) % 3], r % 2, 1, [n]) for r in range(3) for n in range(N)]
    return _one_candidate_each(_cluster(N), _running(jobs), _resv(rows), now, Q, drows)


def four_passes(shape, Q: int | None = None) -> Seam:
    """last_q_of(3) + 1 earliest-start queries of one candidate each on 64 nodes without a reservation (one event slot each), 64 distinct
    queries tiled."""
    if Q is None:
        Q = last_q_of(3) + 1
    N, now = 64, NOW
    base = (now // GRID + 1) * GRID
    jobs = [((base + GRID * (n % 13), INF)[n % 16 == 9], [n]) for n in range(N) if n % 4]
    drows = [(base + GRID * (n % 5) + (0, 1, -1)[n % 3], (1, GRID)[n % 2], 1, 1, [n]) for n in range(N)]
    return _one_candidate_each(_cluster(N), _running(jobs), None, now, Q, drows)


# ---- many_tiles ----------------------------------------------------------------------------------------------------------------------
MANY_NODES = 4096
MANY_RESV_PER_NODE = 3


def many_tiles(shape, extra_queries: int = 0) -> Seam:
    """More than scan_span * sort_tile event times: 4 096 nodes with 3 reservations each, and as many earliest-start queries over ALL
    nodes as it takes (+ extra_queries).  Ends from 8 distinct times (the reference stays cheap), a distinct k per query."""
    rng = np.random.default_rng(0x7117E5)
    N, now = MANY_NODES, NOW
    base = (now // GRID + 1) * GRID
    times = [base + GRID * t for t in (0, 1, 2, 4, 6, 9, 13, 18)]
    rows = []
    for v in range(24):                                                           # node n is listed by v = n % 8, 8 + (n / 8) % 8 and 16 + (n / 64) % 8
        a, b = sorted(int(x) for x in rng.choice(8, 2, replace=False))
        grp, div = v // 8, (1, 8, 64)[v // 8]
        rows.append((times[a] + (0, 0, 1, -1)[v % 4], times[b] if v != 13 else INF, [n for n in range(N) if (n // div) % 8 == v - 8 * grp]))
    jobs = [(times[int(rng.integers(0, 8))], [(j * 5) % N]) for j in range(600)]
    per_query = N * (1 + MANY_RESV_PER_NODE)
    need = shape.scan_span * shape.sort_tile // 2 + 1                             # intervals: two event times each
    Q = (need + per_query - 1) // per_query + extra_queries
    qrows = []
    for i in range(Q):
        cand = [int(x) for x in np.roll(np.arange(N), -131 * i)]
        qrows.append((times[i % 4] + i % 3 - 1, (1, GRID + 1)[i % 2], 100 + 97 * i, 1, cand))
    return Seam(_cluster(N), _running(jobs), _resv(rows), _queries(qrows), now)


# ---- shared, computed once -----------------------------------------------------------------------------------------------------------
BUILDERS = {
    "wide_times": wide_times,
    "dense_nodes": dense_nodes,
    "empties": empties,
    "empties_all_past": lambda shape: empties(shape, "all_past"),
    "three_passes": three_passes,
    "two_passes": lambda shape: three_passes(shape, last_q_of(2)),
    "four_passes": four_passes,
    "three_passes_most": lambda shape: four_passes(shape, last_q_of(3)),
    "many_tiles": many_tiles,
    "many_tiles_more": lambda shape: many_tiles(shape, 2),
}


def shape():
    from cranesched_amd import engine
    return engine.resvq_shape()


@functools.lru_cache(maxsize=None)
def case(name: str) -> Seam:
    return BUILDERS[name](shape())


@functools.lru_cache(maxsize=None)
def expected_of(name: str) -> dict:
    seam = case(name)
    return expected(state_of(seam), seam.now, seam.queries)
