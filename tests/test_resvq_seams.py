"""Do the seam scenarios of tests/resvq_seams.py hit what they name?  Asserted on the inputs, on a statement-by-statement walk of
k_rq_emit (tests/test_resvq_sweep_model.py) and on the answers of the restatement tests/resvq_pyref.py — no GPU.  The device runs the
same scenarios in tests/test_gpu_resvq_seams.py."""
import time

import numpy as np
import pytest

from tests import resvq_pyref as ref
from tests import resvq_seams as rs
from tests.test_resvq_sweep_model import sweep

INF, INT64_MIN = rs.INF, rs.INT64_MIN
CPU_CASES = [n for n in rs.BUILDERS if n not in ("four_passes", "three_passes_most")]   # those two: 8 M queries, the GPU test's business


@pytest.fixture(scope="module")
def answers(built):
    """The reference's answers of every scenario but the 8 M-query ones, and the CPU seconds they took."""
    t0 = time.process_time()
    out = {name: rs.expected_of(name) for name in CPU_CASES}
    return out, time.process_time() - t0


def lists_of(q):
    return [[int(x) for x in q.cand_nodes[int(q.cand_offsets[i]):int(q.cand_offsets[i + 1])]] for i in range(q.num_queries)]


def live_earliest(seam):
    q = seam.queries
    return (q.find_earliest != 0) & (q.start_sec + q.duration_sec > seam.now)      # (the sum fits: the call refuses one that does not)


def intervals(seam):
    """Event slots of the call as resvq_host.inc counts them: per found candidate of a live earliest-start query 1 + the node's reservations."""
    q, N = seam.queries, seam.cluster.num_nodes
    cnt = np.zeros(N + 1, np.int64)
    if seam.resv is not None:
        np.add.at(cnt, seam.resv.alloc_node.astype(np.int64), 1)
    per_cand = np.where(q.cand_nodes < N, 1 + cnt[np.minimum(q.cand_nodes.astype(np.int64), N)], 0)
    return int((per_cand * np.repeat(live_earliest(seam), np.diff(q.cand_offsets.astype(np.int64)))).sum())


def walk(state, n, start, d):
    """k_rq_emit for one found candidate, with the equalities it meets: -> (plus, minus, seen, saturated)."""
    plus, minus, seen, saturated = [], [], set(), False
    cur = max(max(state.job_ends[n], default=INT64_MIN), start)
    alive = cur != INF
    for st, ed in sorted(state.resv[n]):
        if not alive:
            break
        if st == INF:
            seen.add("st == never")
            continue
        saturated |= st - (d - 1) < INT64_MIN
        a = max(st - (d - 1), INT64_MIN, start)
        if a == start and st - (d - 1) < start:
            seen.add("clamped to the start")
        if ed <= a:
            if ed == a:
                seen.add("ed == a")
            continue
        if a > cur:
            plus.append(cur)
            minus.append(a)
        elif a == cur:
            seen.add("a == cur")
        if ed == cur:
            seen.add("ed == cur")
        cur = max(cur, ed)
        alive = cur != INF
        if not alive:
            seen.add("closed by an end at never")
    if alive:
        plus.append(cur)
    return plus, minus, seen, saturated


def walks(seam):
    state = rs.state_of(seam)
    q, live = seam.queries, live_earliest(seam)
    for i, cand in enumerate(lists_of(q)):
        if live[i]:
            for n in cand:
                if n < state.num_nodes:
                    yield i, n, walk(state, n, int(q.start_sec[i]), int(q.duration_sec[i]))


def test_wide_times_covers_the_signed_range(built):
    seam = rs.case("wide_times")
    assert seam.now == -(1 << 62)
    q, state = seam.queries, rs.state_of(seam)
    assert q.num_queries <= 64 and np.diff(q.cand_offsets.astype(np.int64)).max() == rs.shape().pick_block // 4 + 1 <= 65
    times, seen, saturated = [], set(), 0
    for _, _, (plus, minus, s, sat) in walks(seam):
        times += plus + minus
        seen |= s
        saturated += sat
    keys = np.array([(t + (1 << 63)) for t in times], np.uint64)           # rq_key: t ^ 2^63, as an unsigned number
    for byte in range(8):
        assert len(set(((keys >> np.uint64(8 * byte)) & np.uint64(255)).tolist())) >= 3, f"key byte {byte} takes fewer than 3 values"
    both = lambda xs: min(xs) < 0 < max(xs)
    ends = [e for n in range(state.num_nodes) for e in state.job_ends[n]]
    rst = [st for n in range(state.num_nodes) for st, _ in state.resv[n]]
    red = [ed for n in range(state.num_nodes) for _, ed in state.resv[n]]
    assert both(ends) and both(rst) and both(red) and both(q.start_sec.tolist()) and both(times)
    assert any(INT64_MIN < e < INT64_MIN + 100 for e in ends) and INT64_MIN in ends and INF in ends
    assert INT64_MIN in rst and INF in rst and INF in red
    assert any(st != INF and ed == INF for n in range(state.num_nodes) for st, ed in state.resv[n])
    durs = set(q.duration_sec.tolist())
    assert 1 in durs and rs.BIG_DURATION in durs and INF in durs
    assert saturated >= 20, "st - (d - 1) below INT64_MIN in a walked candidate"
    assert {"st == never", "clamped to the start", "closed by an end at never"} <= seen


def test_dense_nodes_meets_every_equality_of_the_merge(built):
    seam = rs.case("dense_nodes")
    q, state = seam.queries, rs.state_of(seam)
    assert 120 <= state.num_nodes <= 140 and all(len(state.resv[n]) == rs.DENSE_RESV_PER_NODE == 40 for n in range(state.num_nodes))
    count = {}
    for i, n, (_, _, s, _) in walks(seam):
        for what in s:
            count[(what, int(q.duration_sec[i]))] = count.get((what, int(q.duration_sec[i])), 0) + 1
    for what in ("a == cur", "ed == a", "ed == cur"):
        for d in (1, rs.GRID, rs.GRID + 1):
            if what == "a == cur" and d == rs.GRID:
                continue                          # (on this grid a duration of 600 leaves one free second instead: the "one off" side)
            assert count.get((what, d), 0) >= 10, (what, d, count)
    mine = sorted(state.resv[rs.DENSE_INF_NODE])
    at = [i for i, (_, ed) in enumerate(mine) if ed == INF]
    assert len(at) == 1 and 5 < at[0] < len(mine) - 5, "an end at INT64_MAX in the middle of the sorted list"
    assert sum(rs.DENSE_INF_NODE in c for c, e in zip(lists_of(q), live_earliest(seam)) if e) >= 2
    # the menu: identical twice, nested, overlapping, disjoint on one node
    for n in range(state.num_nodes):
        r = sorted(state.resv[n])
        pairs = list(zip(r, r[1:]))
        assert any(a == b for a, b in pairs) or any(a[0] < b[0] and b[1] <= a[1] for a, b in pairs) or any(a[0] < b[0] < a[1] < b[1] for a, b in pairs)
    assert set(q.duration_sec.tolist()) == {1, rs.GRID, rs.GRID + 1}
    assert set((q.start_sec % rs.GRID).tolist()) == {0, 1, rs.GRID - 1}
    assert set(np.diff(q.cand_offsets.astype(np.int64)).tolist()) == {rs.shape().pick_block // 4 + 1}
    assert set(q.find_earliest.tolist()) == {0, 1}
    nf_at_start = np.array([ref.at_start(state, int(q.start_sec[i]), int(q.duration_sec[i]), 0, c)[1] for i, c in enumerate(lists_of(q))])
    assert (q.node_num == nf_at_start).sum() >= 20 and (q.node_num == nf_at_start + 1).sum() >= 20


def test_empties(built):
    grid = rs.shape().pick_grid
    seam = rs.case("empties")
    q = seam.queries
    lens = np.diff(q.cand_offsets.astype(np.int64))
    Q = q.num_queries
    assert Q == 2 * grid + 1
    empty = lens == 0
    assert empty[:3].all() and empty[-3:].all() and empty[Q // 2:Q // 2 + 4].all() and not empty[3] and not empty[-4]
    for run in (slice(0, 3), slice(Q // 2, Q // 2 + 4), slice(Q - 3, Q)):
        assert set(q.node_num[run].tolist()) == {0, 5} and set(q.find_earliest[run].tolist()) == {0, 1}
    N = seam.cluster.num_nodes
    ghosts_only = [i for i, c in enumerate(lists_of(q)) if c and min(c) >= N and q.find_earliest[i]]
    assert ghosts_only and all(live_earliest(seam)[i] for i in ghosts_only)
    jobs = np.diff(seam.running.alloc_offsets.astype(np.int64)) == 0
    assert jobs[0] and jobs[-1] and (jobs[1:-1][:-1] & jobs[1:-1][1:]).any() and not jobs.all()
    past = rs.case("empties_all_past")
    pq = past.queries
    assert (pq.find_earliest != 0).any() and not live_earliest(past).any() and intervals(past) == 0
    assert ((pq.find_earliest == 0) & (pq.start_sec + pq.duration_sec > past.now)).any()


def test_every_status_and_code_occurs_and_some_queries_wait(answers):
    exp, _ = answers
    status, codes = set(), set()
    for name in CPU_CASES:
        status |= set(exp[name]["status"].tolist())
        codes |= set(exp[name]["code"].tolist())
    assert status == {ref.OK, ref.NOT_ENOUGH, ref.IN_THE_PAST} and codes == {ref.FREE, ref.RUNNING, ref.RESERVED, ref.NOT_FOUND}
    for name in ("wide_times", "dense_nodes", "many_tiles", "three_passes"):
        q = rs.case(name).queries
        later = (q.find_earliest != 0) & (exp[name]["status"] == ref.OK) & (exp[name]["start_sec"] > q.start_sec)
        assert later.sum() >= 5, name
    for name in ("wide_times", "dense_nodes"):                   # both modes, each with a yes and a no
        q = rs.case(name).queries
        assert set(zip(q.find_earliest.tolist(), exp[name]["status"].tolist())) >= {(m, s) for m in (0, 1) for s in (ref.OK, ref.NOT_ENOUGH)}, name
    k = rs.case("many_tiles").queries.node_num
    assert len(set(k.tolist())) == len(k), "a distinct k per query"
    assert len(set(exp["many_tiles"]["start_sec"].tolist())) >= 3, "the answers differ between the segments"


def test_each_scenario_lies_on_its_side_of_the_constants(built):
    s = rs.shape()
    one_step = s.scan_span * s.sort_tile                           # event times one step of the sort's scan covers
    assert rs.digit_bits() == 8
    sizes = {name: rs.case(name).queries.num_queries for name in CPU_CASES}
    assert sizes["two_passes"] + 1 == sizes["three_passes"] == rs.last_q_of(2) + 1
    assert rs.seg_passes(sizes["two_passes"]) == 2 and rs.seg_passes(sizes["three_passes"]) == 3
    assert rs.seg_passes(rs.last_q_of(3)) == 3 and rs.seg_passes(rs.last_q_of(3) + 1) == 4 and rs.last_q_of(3) == 8_388_608
    assert rs.seg_passes(rs.last_q_of(1)) == 1 and rs.seg_passes(rs.last_q_of(1) + 1) == 2 and rs.last_q_of(2) == 32_768
    for name in ("wide_times", "dense_nodes", "empties_all_past"):
        assert rs.seg_passes(sizes[name]) == 1, name
    assert rs.seg_passes(sizes["empties"]) == 2 and sizes["empties"] > 2 * s.pick_grid
    ev = {name: intervals(rs.case(name)) for name in CPU_CASES}
    tiles = {name: (2 * ev[name] + s.sort_tile - 1) // s.sort_tile for name in CPU_CASES}
    assert 2 * ev["many_tiles"] > one_step and tiles["many_tiles"] > s.scan_span and 2 * (ev["many_tiles"] - rs.MANY_NODES * 4) <= one_step, "the fewest queries that cross"
    assert tiles["many_tiles_more"] > tiles["many_tiles"]
    for name in ("wide_times", "dense_nodes", "empties", "two_passes", "three_passes"):
        assert 1 <= tiles[name] <= s.scan_span, (name, tiles[name])
    assert tiles["dense_nodes"] > 1 and tiles["three_passes"] > 1
    assert ev["three_passes"] >= sizes["three_passes"] - 1000       # (almost) every query sorts event times of its own
    assert 2 * (rs.last_q_of(3) + 1) > one_step                     # four_passes: one slot per query, also beyond one step of the scan


def test_the_sweep_model_agrees_on_the_seams(answers):
    """The Python model of the device's sweep (k_rq_emit, the sort, k_rq_first) gives the brute force's earliest start on the scenarios
    that stress the merge and the ends of time: the ALGORITHM holds there, whatever the device makes of it."""
    exp, _ = answers
    checked = 0
    for name in ("wide_times", "dense_nodes", "empties"):
        seam = rs.case(name)
        state, q, live = rs.state_of(seam), seam.queries, live_earliest(seam)
        for i, cand in enumerate(lists_of(q)):
            if not live[i]:
                continue
            t = sweep(state, int(q.start_sec[i]), int(q.duration_sec[i]), int(q.node_num[i]) or len(cand), cand)
            if exp[name]["status"][i] == ref.OK:
                assert t == int(exp[name]["start_sec"][i]), (name, i)
            else:
                assert t is None, (name, i)
            checked += 1
    assert checked > 400


def test_the_reference_alone_is_quick(answers):
    _, seconds = answers
    assert seconds < 60, f"the reference took {seconds:.1f} s of CPU for the scenarios"


def test_expected_replicates_the_plain_answer(built):
    """expected() — once per distinct query, then replicated — is resvq_pyref.answer itself on a scenario small enough to do both."""
    seam = rs.case("empties")
    plain = ref.answer(rs.state_of(seam), seam.now, seam.queries)
    for f, a in rs.expected_of("empties").items():
        assert a.dtype == plain[f].dtype and np.array_equal(a, plain[f]), f
    rep, inv = rs.distinct(seam.queries)
    assert len(rep) < seam.queries.num_queries and len(inv) == seam.queries.num_queries
