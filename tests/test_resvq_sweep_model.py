"""A Python model of the earliest-start sweep of csrc/resvq_kernels.inc (k_rq_emit, the two sorts, k_rq_first), statement by statement,
against the brute force of tests/resvq_pyref.py on the scenarios of the GPU tests: the algorithm is checked where no GPU is."""
import bisect

import numpy as np

from tests import resvq_case as rc
from tests import resvq_pyref as ref

NEVER = ref.INT64_MAX
INT64_MIN = -(1 << 63)


def emit(state, n, start, d):
    """k_rq_emit for one found candidate: (plus times, minus times)."""
    plus, minus = [], []
    le = max(state.job_ends[n], default=INT64_MIN)
    cur = max(le, start)
    alive = cur != NEVER
    for st, ed in sorted(state.resv[n]):
        if not alive:
            break
        if st == NEVER:
            continue
        a = max(max(st - (d - 1), INT64_MIN), start)
        if ed <= a:
            continue
        if a > cur:
            plus.append(cur)
            minus.append(a)
        cur = max(cur, ed)
        alive = cur != NEVER
    if alive:
        plus.append(cur)
    assert len(plus) <= 1 + len(state.resv[n]) and len(minus) <= len(state.resv[n])
    return plus, minus


def sweep(state, start, d, k, cand):
    """-> the least t with at least k free candidates, or None (k_rq_first over the sorted event times)."""
    if k == 0:
        return start
    plus, minus = [], []
    for n in cand:
        if n < state.num_nodes:
            p, m = emit(state, n, start, d)
            plus += p
            minus += m
    plus.sort()
    minus.sort()
    best = None
    for i, t in enumerate(plus):
        if i + 1 < len(plus) and plus[i + 1] == t:
            continue
        if (i + 1) - bisect.bisect_right(minus, t) >= k:
            best = t if best is None else min(best, t)
    return best


def test_sweep_equals_brute_force():
    checked = waits = never = 0
    for seed in range(12):
        cluster, running, resv, times = rc.random_cluster(seed, None if seed % 3 else 40)
        state = ref.NodeState(cluster.num_nodes, running, resv)
        q = rc.random_queries(seed, cluster.num_nodes, state, times, 48, lengths=(1, 2, 5, 17, 64, 130))
        for i in range(q.num_queries):
            cand = [int(x) for x in q.cand_nodes[int(q.cand_offsets[i]):int(q.cand_offsets[i + 1])]]
            start, d = int(q.start_sec[i]), int(q.duration_sec[i])
            for k in {int(q.node_num[i]) or len(cand), 1, 2, max(1, len(cand) // 2)}:
                want = ref.earliest(state, start, d, k, cand)[0]
                assert sweep(state, start, d, k, cand) == want, (seed, i, k)
                checked += 1
                waits += want is not None and want > start
                never += want is None
    assert checked > 1000 and waits > 50 and never > 50


def test_sweep_at_the_ends_of_time():
    """Saturation: a start near INT64_MAX, reservations that begin at INT64_MIN or never, durations that reach past the end."""
    s = ref.NodeState(4)
    s.resv[0] = [(INT64_MIN, INT64_MIN + 5), (NEVER - 3, NEVER - 1)]
    s.resv[1] = [(NEVER, NEVER)]
    s.resv[2] = [(NEVER - 100, NEVER - 50), (NEVER - 60, NEVER - 40)]
    s.job_ends[3] = [NEVER - 20]
    for start, d in ((NEVER - 200, 10), (NEVER - 200, 199), (NEVER - 45, 40), (INT64_MIN, 3), (INT64_MIN + 4, NEVER), (0, NEVER)):
        for k in (1, 2, 3, 4):
            for cand in ([0, 1, 2, 3], [3, 2], [1], [0]):
                assert sweep(s, start, d, k, cand) == ref.earliest(s, start, d, k, cand)[0], (start, d, k, cand)
