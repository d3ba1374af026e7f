"""Cases on the seams of TryPreempt_'s device form (cranesched_amd/csrc/preempt_dev.inc), built from the sizes it is compiled with
(cns_preempt_shape: sort_lanes, rank_sort_max, compact_records, cache_nodes, pool_nodes).  No HIP in here and no random numbers: the only
disorder is one fixed permutation of the running jobs' ledger order, so that the device's sort has work to do.  Expected values never
come from this file: tests/test_preempt_seams.py holds the oracle to tests/select_pyref.py on every case and asserts, from pyref's
recorder and from the device's own tree source replayed on the CPU (tests/host_seg/seg_host.cpp --replay), the CONDITION each builder's
docstring states — the reason the case is a test of its seam; tests/test_gpu_preempt_seams.py holds the engine to the oracle.

The common frame: one partition (two where stated), nodes of 64 cores whose memory is the contended resource, allocations of one raw cpu
unit (1/256 core: no core ids) and 1..4 GiB, QoS 0 ("low") preemptible by QoS 1 ("high"), QoS 2 ("fixed") neither.  A preemptor asks for
one raw cpu unit and W GiB on each of its nodes for 100 s; every low job outlasts that window unless stated, so its trees stay one node
deep and the case is about the candidates: how many, in which order, from where."""
from __future__ import annotations

import numpy as np

from cranesched_amd import abi

GIB = 1 << 30
NOW = 1000
END = NOW + 5000          # the running jobs' end: past every preemptor's window
LOW, HIGH, FIXED = 0, 1, 2
QOS_PREEMPT = [[], [LOW], []]
QPRIO = {LOW: 10, HIGH: 30, FIXED: 20}
CORES = 64


def ledger_order(n):
    """The fixed permutation: position -> which of n rows stands there.  Not monotone, no fixed run longer than one."""
    return sorted(range(n), key=lambda i: ((i * 37 + 11) % 101, (i * 7) % 13, i))


_CACHE = {}
# the case list at the shipped shape (64, 256, 251, 512, 65536): pytest parametrizes over it, tests/test_preempt_seams.py holds it to case_names()
CASE_NAMES = ["nc_1", "nc_63", "nc_64", "nc_65", "nc_128", "nc_255", "nc_256", "nc_257", "nc_320", "ties_running", "ties_pending", "ties_mix",
              "multi_k2", "multi_k3", "multi_k17", "list_63", "list_64", "list_65", "list_129", "pending_again", "shared_130", "compact_full",
              "compact_over", "pool_deep", "pool_over"]


class Frame:
    """Collects nodes, running jobs and queue jobs; build() -> (cluster, jobs, now, running, preempt)."""

    def __init__(self, node_mem_gib, parts=None):
        self.node_mem = list(node_mem_gib)
        self.parts = parts or [list(range(len(self.node_mem)))]
        self.rn, self.pd = [], []
        self.preempting = []

    def run(self, allocs, start, qos=LOW, qprio=None, end=END):
        """A running job: allocs = [(node, GiB)], -> its position in the list handed to build() (NOT its ledger row)."""
        self.rn.append(dict(allocs=list(allocs), start=start, qos=qos, qprio=QPRIO[qos] if qprio is None else qprio, end=end))
        return len(self.rn) - 1

    def job(self, gib, qos, nodes, L=100, prio=None, part=0, qprio=None):
        """A queue job: gib on each of len(nodes) nodes, confined to them (include list).  -> its queue index."""
        self.pd.append(dict(gib=gib, qos=qos, nodes=list(nodes), L=L, prio=float(len(self.pd)) + 0.5 if prio is None else float(prio), part=part,
                            qprio=QPRIO[qos] if qprio is None else qprio))
        return len(self.pd) - 1

    def fill(self, extra=None):
        """Every node's memory = what runs on it (nothing free), plus extra[node] GiB."""
        tot = [0] * len(self.node_mem)
        for r in self.rn:
            for n, g in r["allocs"]:
                tot[n] += g
        for n in range(len(tot)):
            self.node_mem[n] = tot[n] + (extra or {}).get(n, 0)

    def build(self, permute=True):
        n = len(self.node_mem)
        off = np.cumsum([0] + [len(p) for p in self.parts]).astype(np.uint32)
        full = np.uint64((1 << CORES) - 1) if CORES < 64 else np.uint64(0xFFFFFFFFFFFFFFFF)
        c = abi.Cluster(np.full(n, CORES * 256, np.int64), np.asarray([max(g, 1) * GIB for g in self.node_mem], np.uint64), np.full(n, full, np.uint64),
                        np.zeros(n, np.uint64), np.zeros(n, np.uint64), off, np.concatenate([np.asarray(p, np.uint32) for p in self.parts]))
        order = ledger_order(len(self.rn)) if permute else list(range(len(self.rn)))
        self.row_of = {src: row for row, src in enumerate(order)}
        rows = [self.rn[i] for i in order]
        aoff, node, mem = [0], [], []
        for r in rows:
            for nd, g in r["allocs"]:
                node.append(nd); mem.append(g * GIB)
            aoff.append(len(node))
        z = np.zeros(len(node), np.uint64)
        run = abi.Running(np.asarray([r["end"] for r in rows], np.int64), np.asarray(aoff, np.uint32), np.asarray(node, np.uint32),
                          np.ones(len(node), np.int64), np.asarray(mem, np.uint64), z, z.copy(), z.copy()) if rows else None
        J = len(self.pd)
        ioff, inodes = [0], []
        for p in self.pd:
            inodes += p["nodes"]
            ioff.append(len(inodes))
        k = np.asarray([len(p["nodes"]) for p in self.pd], np.uint32)
        j = abi.Jobs(partition=np.asarray([p["part"] for p in self.pd], np.uint32), time_limit_sec=np.asarray([p["L"] for p in self.pd], np.int64),
                     node_mem=np.zeros(J, np.uint64), task_cpu_raw=np.ones(J, np.int64), task_mem=np.asarray([p["gib"] * GIB for p in self.pd], np.uint64),
                     node_num=k, ntasks=k.copy(), ntasks_per_node_min=np.ones(J, np.uint32), ntasks_per_node_max=np.ones(J, np.uint32),
                     incl_offsets=np.asarray(ioff, np.uint64), incl_nodes=np.asarray(inodes, np.uint32))
        ids = 1000 + np.arange(len(rows))
        pre = abi.Preempt(QOS_PREEMPT, 1 + np.arange(J), [p["qos"] for p in self.pd], [p["qprio"] for p in self.pd], [p["prio"] for p in self.pd],
                          ids, [r["qos"] for r in rows], [r["qprio"] for r in rows], [r["start"] for r in rows],
                          preempting=[int(ids[self.row_of[i]]) for i in self.preempting])
        return c, j, NOW, run, pre


class Case:
    """name, the inputs, and `want`: what tests/test_preempt_seams.py asserts of the recorder and the replay (test_the_case_meets_its_condition there): a dict
    call number (in the cycle's order of TryPreempt_ calls that had candidates) -> requirements, plus case-wide keys."""

    def __init__(self, name, frame, want, doc, permute=True):
        self.name, self.want, self.doc = name, want, doc
        self.inputs = frame.build(permute)
        self.frame = frame


def sizes_for(nc, applied):
    """Candidate sizes in the order the comparator gives them: 1 / 2 / 1 GiB ... , the `applied`-th candidate 3 GiB, and the demand
    W that the first applied - 1 miss by one GiB: the forward pass stops at the large one with 2 GiB to spare, the pass back drops the
    small one in front of it, keeps the 2 GiB one before that (1 GiB to spare is not enough) and drops the next small one."""
    s = [2 if x % 3 == 1 else 1 for x in range(nc)]
    if applied >= 1:
        s[applied - 1] = 3 if applied > 1 else 1
    w = sum(s[:applied - 1]) + 1
    return s, w


def applied_for(nc):
    return nc if nc < 3 else nc - max(1, nc // 8)


def low_jobs_on(f, node, sizes, first_start=NOW - 1):
    """Running low jobs on `node`, handed over in the comparator's order: equal qos_priority, the later start first."""
    return [f.run([(node, g)], first_start - x) for x, g in enumerate(sizes)]


def nc_case(shape, nc):
    """nc_<n>: one node, n candidates, one preemptor.  CONDITION: call 0 has exactly n candidates and 0 < chosen < applied < n
    (n == 1 cannot: there chosen == applied == 1).  At n == sort_lanes and sort_lanes + 1 a second preemptor on a second node with n
    candidates of its own needs every one of them: it is satisfied after exactly n applications — apply()'s last candidate from the
    lane registers, and its first one from memory."""
    f = Frame([0, 0])
    a = applied_for(nc)
    s, w = sizes_for(nc, a)
    low_jobs_on(f, 0, s)
    want = {0: dict(candidates=nc, applied=a, strict=nc >= 3)}
    f.job(w, HIGH, [0])
    if nc in (shape.sort_lanes, shape.sort_lanes + 1):
        low_jobs_on(f, 1, [1] * nc, first_start=NOW - 500)
        f.job(nc, HIGH, [1])
        want[1] = dict(candidates=nc, applied=nc, chosen=nc)
    else:
        f.run([(1, 1)], NOW - 900, qos=FIXED)
    f.fill()
    return Case(f"nc_{nc}", f, want, nc_case.__doc__)


def ties_case(shape, kind):
    """ties_<kind>: 2 * sort_lanes + 2 candidates whose keys are equal in runs of three, so that two runs straddle a 64-lane chunk of the
    rank sort; the comparator falls through to the ascending index, which the ledger's permutation (running) and the queue's order
    (pending) make unrelated to the position.  running: equal (qos_priority, start); pending: start-now queue jobs with equal
    (qos_priority, priority); mix: members of the preempting set, pending and running jobs, each group with such runs.  CONDITION: call 0
    has that many candidates, 0 < chosen < applied < candidates, and in its sorted order the candidates at positions sort_lanes - 1 |
    sort_lanes and 2 * sort_lanes - 1 | 2 * sort_lanes have equal keys (index apart)."""
    n = 2 * shape.sort_lanes + 2
    f = Frame([0])
    gib = lambda i: 1 + (i * 5) % 3
    if kind == "running":
        for x in range(n):
            f.run([(0, gib(x))], NOW - 1 - x // 3)
        f.fill()
    elif kind == "pending":
        f.run([(0, 1)], NOW - 900, qos=FIXED)
        f.fill({0: sum(gib(i) for i in range(n))})
        spread = sorted(range(n), key=lambda i: ((i * 29) % 31, i))     # queue position -> rank of its priority
        for i in range(n):
            f.job(gib(i), LOW, [0], L=5000, prio=float(spread[i] // 3))
    else:
        a, b = shape.sort_lanes - 2, shape.sort_lanes + 1                # the preempting set ends at position 61, the pending jobs at 126
        for x in range(a):
            f.preempting.append(f.run([(0, gib(x))], NOW - 1 - x // 3))
        f.run([(0, 1)], NOW - 900, qos=FIXED)
        for x in range(n - a - b):
            f.run([(0, gib(x + 1))], NOW - 1 - x // 3)
        f.fill({0: sum(gib(i + 2) for i in range(b))})
        spread = sorted(range(b), key=lambda i: ((i * 29) % 31, i))
        for i in range(b):
            f.job(gib(i + 2), LOW, [0], L=5000, prio=float(spread[i] // 3))
    others = sum(g for x, r in enumerate(f.rn) if r["qos"] == LOW and x not in f.preempting for _, g in r["allocs"]) + sum(p["gib"] for p in f.pd)
    given = sum(g for x in f.preempting for _, g in f.rn[x]["allocs"])   # (a member of the preempting set ends at now + 1: free from then on anyway)
    find_demand(f, [0], range(given + (others * 3) // 4, given, -1))
    return Case(f"ties_{kind}", f, {0: dict(candidates=n, strict=True, tie_at=[shape.sort_lanes, 2 * shape.sort_lanes])}, ties_case.__doc__)


def find_demand(f, nodes, demands, **kw):
    """Appends the preemptor to the queue: the first of `demands` (GiB per node) with which its call chooses fewer candidates than it
    applied and applies fewer than there are — found with tests/select_pyref.py's recorder, the engine has no part in it."""
    me = f.job(1, HIGH, nodes, **kw)
    for w in demands:
        f.pd[me]["gib"] = w
        calls = [r for r in call_ops(f.build())[0] if r["job"] == me]
        if calls and calls[0]["chosen"] is not None and 0 < len(calls[0]["chosen"]) < calls[0]["applied"] < calls[0]["candidates"]:
            return me
    raise AssertionError("no demand gives 0 < chosen < applied < candidates")


def multi_case(shape, k):
    """multi_k<k>: a preemptor over k nodes.  Every one of the k nodes lists sort_lanes + 2 one-node low jobs, so that past the first node
    the duplicate test of the collection works on more than 64 candidates whichever node comes first; the candidates with the latest
    starts (the first to be applied) hold two allocations: on two of the k nodes, or on one of them and on a node outside.  CONDITION:
    call 0 has k trees, more than sort_lanes candidates on its first node, among the first sort_lanes candidates of its order jobs with two
    allocations inside the k nodes and jobs with one inside and one outside, every candidate once, and 0 < chosen < applied <
    candidates.  k == 2, 3 stay within rank_sort_max candidates, k == 17 goes past it."""
    outside = [k, k + 1]
    f = Frame([0] * (k + 2))
    x = 0
    for i in range(k):                                   # two allocations inside
        f.run([(i, 2), ((i + 1) % k, 1)], NOW - 1 - x); x += 1
    for i in range(k):                                   # one inside, one outside
        f.run([(i, 1), (outside[i % 2], 3)], NOW - 1 - x); x += 1
    own = shape.sort_lanes + 2
    for t in range(own):
        for i in range(k):
            f.run([(i, 1 + (t + i) % 3)], NOW - 1 - x); x += 1
    for o in outside:
        f.run([(o, 1)], NOW - 900, qos=FIXED)
    f.fill()
    per_node = min(sum(g for r in f.rn for n, g in r["allocs"] if n == i) for i in range(k))
    f.job((per_node * 2) // 3, HIGH, list(range(k)))
    nc = 2 * k + own * k
    return Case(f"multi_k{k}", f, {0: dict(candidates=nc, strict=True, trees=k, first_node_over=shape.sort_lanes, two_inside=True, in_and_out=True)},
                multi_case.__doc__)


def list_case(shape, n):
    """list_<n>: a node whose running list has n entries and whose chain of pending records has n, every third of them of the listed
    QoS.  The pending records: n queue jobs confined to the node ahead of the preemptors, most start now, the last ones of each QoS are
    too large for what is left and are backfilled behind the running jobs' end.  A first preemptor takes some running and some pending
    jobs (gone for the second: entries and records marked in the middle of a 64-entry step), a second one follows.  CONDITION: n running
    entries and n placed queue jobs on the node; call 0 has their listed third as candidates and chooses both kinds; call 1 has
    call 0's candidates less the running jobs and the start-now queue jobs it chose, and chooses some."""
    f = Frame([0])
    listed = lambda i: i % 3 == 1
    for x in range(n):
        f.run([(0, 1 + x % 2)], NOW - 1 - x, qos=LOW if listed(x) else FIXED)
    big = 6
    small = sum(1 for i in range(n - big))
    f.fill({0: small})
    for i in range(n):
        late = i >= n - big
        f.job(n + 5 if late else 1, LOW if listed(i) else FIXED, [0], L=6000 + i, prio=float((i * 29) % 31))
    cand = sum(1 for i in range(n) if listed(i))
    low_run = sum(1 + x % 2 for x in range(n) if listed(x))
    low_now = sum(1 for i in range(n - big) if listed(i))   # the listed start-now queue jobs come first in the order: ask for more than they hold
    f.job(low_now + max(2, low_run // 2), HIGH, [0])
    f.job(max(2, low_run // 4), HIGH, [0])
    return Case(f"list_{n}", f, {0: dict(candidates=2 * cand, both_kinds=True), 1: dict(after=0), "node_lists": (0, n, n)}, list_case.__doc__)


def pending_again_case(shape):
    """pending_again: a backfilled low job is preempted and stays in the node's job list (only a job that was scheduled to start now
    is taken out), so the next preemptor is offered it and takes it AGAIN; a start-now low job is preempted too (reason 7, not among the
    cancelled).  Node of 20 GiB: F0 (fixed) holds 6 until now + 50.  P0 (low, 6 GiB, 80 s) starts now; P1 (low, 12 GiB) is backfilled at
    now + 50; A (high, 9 GiB, 100 s) needs P1 for [50, 100) and P0 for [0, 50): both chosen.  P2 (fixed, 10 GiB) is backfilled at now + 50
    into what they gave back; B (high, 4 GiB, 100 s) fits [0, 50) but not [50, 100): P1, still listed, is chosen again.  CONDITION: call
    0 chooses the pending jobs 0 and 1, call 1's only candidate is the pending job 1 and it is chosen."""
    f = Frame([20])
    f.run([(0, 6)], NOW - 100, qos=FIXED, end=NOW + 50)
    f.job(6, LOW, [0], L=80, prio=2.0)
    f.job(12, LOW, [0], L=1000, prio=1.0)
    f.job(9, HIGH, [0])
    f.job(10, FIXED, [0], L=1000)
    f.job(4, HIGH, [0])
    return Case("pending_again", f, {0: dict(candidates=2, chosen_set=[("pd", 0), ("pd", 1)]), 1: dict(candidates=1, chosen_set=[("pd", 1)]), "reasons": {0: 7, 1: 7}},
                pending_again_case.__doc__)


def shared_case(shape):
    """shared_130: nc_128's frame with 2 * sort_lanes + 2 candidates on a node that two partitions list, so every allocation stands under
    both of the node's slots and is taken once (under the node's first slot).  The first preemptor belongs to the SECOND partition — its
    slot is not the node's first: the lanes' registers hold no tree for its candidates —, the next one to the first partition.
    CONDITION: both calls have candidates; call 0 has 2 * sort_lanes + 2 of them, 0 < chosen < applied < candidates; call 1 has call 0's
    less what it chose."""
    nc = 2 * shape.sort_lanes + 2
    f = Frame([0, 0], parts=[[0, 1], [0]])
    a = applied_for(nc) - 30
    s, w = sizes_for(nc, a)
    low_jobs_on(f, 0, s)
    f.run([(1, 1)], NOW - 900, qos=FIXED)
    f.fill()
    f.job(w, HIGH, [0], part=1)
    f.job(max(2, w // 4), HIGH, [0], part=0)
    return Case("shared_130", f, {0: dict(candidates=nc, applied=a, strict=True), 1: dict(after=0)}, shared_case.__doc__)


# ---- deep trees: the candidates end INSIDE the preemptor's window, one second apart -------------------------------------------
def deep_frame(per_node, nodes, window):
    """Per node `per_node` low jobs of 1 GiB that end at now + 1, now + 2, ... (the later the start, the earlier the end) and nothing
    free: t seconds from now t GiB are.  A fixed queue job per node asks for half the node and is backfilled where that much is free:
    from there on the node is short again.  The preemptor wants 1 GiB on every node for `window` seconds: each tree holds the node's
    whole time map (a range end per second), is short in its first second and in the first second of the backfilled job, and takes
    the candidates in the order of their ends until one reaches past that second — the pass back then drops all the others.
    (A demand above a candidate's size cannot be met on such trees at all: a node that a range covers completely takes `satisfied` from
    its own resource, and an inner node's own resource is only what covered it completely.)"""
    f = Frame([0] * nodes)
    for i in range(nodes):
        for t in range(per_node):
            f.run([(i, 1)], NOW - 1 - t, end=NOW + 1 + t)
    f.fill()
    for i in range(nodes):
        f.job(max(1, per_node // 2), FIXED, [i], L=2 * window)
    f.job(1, HIGH, list(range(nodes)), L=window)
    return f


def call_ops(inputs):
    """The recorded calls of the case (tests/select_pyref.py's recorder)."""
    from tests.test_preempt import run_pyref_preempt
    c, j, now, run, pre = inputs
    rec = []
    cyc, out, lists = run_pyref_preempt(c, j, now, run, pre, recorder=rec)
    return rec, cyc, out, lists


def predicted_use(call):
    """(records, nodes): what the compressed and the node-for-node form need for the call, from their Python descriptions
    (tests/seg_compact.py) — the builders' search uses it, the tests assert the device source's own figures (the replay)."""
    from tests import seg_compact as sc
    k = len(call["targets"])
    R = lambda r: sc.R(cpu=r.cpu, mem=r.mem)
    comp = [sc.CompactTree(0, call["seg_end"], R(t)) for t in call["targets"]]
    lit = [sc.LiteralTree(0, call["seg_end"], R(t)) for t in call["targets"]]
    for ti, _, st, ed, r, plus in call["ops"]:
        comp[ti].op(st, ed, R(r), plus)
        lit[ti].op(st, ed, R(r), plus)

    def records(n):
        if n is None or isinstance(n, sc.Leaf):
            return 0 if n is None else 1
        return 1 + records(n.cl) + records(n.cr)

    def nodes(n):
        c, stack = 0, [n]
        while stack:
            m = stack.pop()
            c += 1
            if m["ls"] is not None:
                stack += [m["ls"], m["rs"]]
        return c
    return sum(records(t.root) for t in comp), sum(nodes(t.root) for t in lit)


def compact_case(shape, over):
    """compact_full / compact_over: one node, candidates ending one second apart inside the window, as many as it takes.  The builder
    takes the largest number of them whose call needs no more than compact_records records (full), and that number and a half (over).
    CONDITION by the replay of the device's tree source: full — C.used within the last tenth below compact_records, no overflow; over —
    the compressed form overflows and cache_nodes < T.used < pool_nodes, no overflow there.  No CNS_PREEMPT_TREE setting is involved."""
    key = ("compact", tuple(shape))
    if key not in _CACHE:
        best = None
        for m in range(shape.compact_records // 3, shape.compact_records, 4):   # (a range end costs about two records)
            used = predicted_use(call_ops(deep_frame(m, 1, 1000).build())[0][0])[0]
            if used > shape.compact_records:
                break
            best = m
        _CACHE[key] = best
    best = _CACHE[key]
    m = best + best // 2 if over else best
    f = deep_frame(m, 1, 1000)
    want = {0: dict(candidates=m, replay="over" if over else "full")}
    return Case("compact_over" if over else "compact_full", f, want, compact_case.__doc__)


NODES_PER_END = 60   # the node-for-node tree's cost of one more range end one second from the last, in a window of about 2^42 ticks: two
                     # nodes per level below the ~10 levels it shares with its neighbour (an estimate; the replay's figures are asserted)


def pool_case(shape, over):
    """pool_deep / pool_over: two nodes, several hundred candidates on each ending one second apart inside the window (fewer than the 1000
    time-map entries at which a node is passed over, and than the engine's 1006 allocations per node).  CONDITION by the replay: deep —
    pool_nodes / 2 < T.used < pool_nodes and no overflow; over — the node-for-node form overflows (the reference's own trees hold more
    than pool_nodes nodes in the end).  pool_over is answered with CNS_ERR_UNSUPPORTED; that is a status, the kernel ends normally."""
    per_node = (shape.pool_nodes * (23 if over else 13) // 20) // (2 * NODES_PER_END)
    assert per_node < 900
    f = deep_frame(per_node, 2, 1000)
    return Case("pool_over" if over else "pool_deep", f, {0: dict(candidates=2 * per_node, trees=2, replay="pool_over" if over else "pool_deep")}, pool_case.__doc__)


def case_names(shape):
    L = shape.sort_lanes
    ncs = sorted({1, L - 1, L, L + 1, 2 * L, shape.rank_sort_max - 1, shape.rank_sort_max, shape.rank_sort_max + 1, shape.rank_sort_max + L})
    lists = sorted({L - 1, L, L + 1, 2 * L + 1})
    return ([f"nc_{n}" for n in ncs] + ["ties_running", "ties_pending", "ties_mix"] + ["multi_k2", "multi_k3", "multi_k17"] + [f"list_{n}" for n in lists] +
            ["pending_again", "shared_130", "compact_full", "compact_over", "pool_deep", "pool_over"])


def case(shape, name):
    """The case of that name for that shape (built once per process)."""
    key = (tuple(shape), name)
    if key not in _CACHE:
        kind, _, arg = name.partition("_")
        if kind == "nc":
            c = nc_case(shape, int(arg))
        elif kind == "ties":
            c = ties_case(shape, arg)
        elif kind == "multi":
            c = multi_case(shape, int(arg[1:]))
        elif kind == "list":
            c = list_case(shape, int(arg))
        elif name == "pending_again":
            c = pending_again_case(shape)
        elif name == "shared_130":
            c = shared_case(shape)
        elif kind == "compact":
            c = compact_case(shape, arg == "over")
        elif kind == "pool":
            c = pool_case(shape, arg == "over")
        else:
            raise KeyError(name)
        assert c.name == name
        _CACHE[key] = c
    return _CACHE[key]
