"""Cases on the seams of the selection kernels (csrc/select_kernels.hip, pipe_kernel.inc, wide_kernel.inc), every size taken from
cns_select_shape (engine.select_shape()).  No HIP in here and no random numbers.  Expected values never come from this file:
tests/test_select_seams.py runs the oracle (and the reference build where there is one) on every case and asserts its CONDITION — a
function of the oracle's answers that states what puts the case on its seam; tests/test_gpu_select_seams.py holds the engine to the
oracle on the same cases.

A case is a Case tuple: (name, cluster, jobs, now, running, cfg, condition) and, behind those, `specs` (the queue as tests/kat.py job
specs: condition(ora) calls ora(n) for the oracle's run of the first n of them, ora() for the whole queue), `nodes` (the seam nodes,
whose final time maps the GPU test compares entry for entry), `covers` (the fields of the shape the case stands on) and `kernel`
(family B: (CNS_SELECT_KERNEL word, what last_kernel() must name)).

Family A — the length of a time map (chunk c = tl_chunk).  The frame: node 0 has 256 cores (64 in the _c64 twin of every case) and R
running allocations of U = 64 (16) raw cpu units (a fraction of a cpu: no core ids) that end G = 100 s apart, so its map has M = R + 2
entries: entry 0 at now, entry i at now + i * G with T - (R - i) * U units free, the last one at infinity with nothing.  A "dip" at
entry e is a queue job in front that asks for all but `leave` of what entry e has, for G seconds: it cannot start earlier (entry
e - 1 has U fewer, the decisive job asks for Y = U / 2), ends on the key of entry e + 1 and so leaves M as it is.  The decisive job
asks for Y units.  The window-end cases are the commit cases too: a start-now commit whose end key exists (win_*_out: M stays) or is
new (spoil_*_up: M + 1), a backfilled commit that inserts both boundaries (t0_*_free: M + 2, the start boundary at index e + 1).
Departures from the issue's wording, forced by the reference's own rules:
  * the ring seams of family D are covered by bursts sized from the shape; a case cannot tell from the oracle which ring slot a task
    took, so their CONDITION states only the burst (every job starts now, the one in the middle waits);
  * entry c - 1 or c can only be dipped where entry e + 1 is a finite key (e <= M - 3); for M = c - 1, c, c + 1 the dip sits at the last
    entry that allows it, e = M - 3 (lanes c - 4 .. c - 2);
  * the last entry of a map is the zero entry at infinity, which no request fits: "a run that starts at lane c - 1 of a map of c
    entries" cannot exist; the nearest is the run that starts at lane c - 2 and ends at the last entry (run_M<c>_e<c-3>_long);
  * an exclusive job needs entries that hold the whole node, which allocations never leave behind them: the keys of the exclusive
    cases come from running allocations of NO resources (they cost nothing and change nothing but the map's length), and the one
    spoiling entry from a two-node job in front that node 1 (busy until then) holds back to exactly that key.  A one-node job that
    is refused now and then backfilled onto the same node gets the same start: a third, cheaper node that is busy for ten seconds
    makes the refusal visible;
Family B — node counts: for every tile of every kernel family, partitions of lanes * w - 1, lanes * w and lanes * w + 1 nodes, all of
one core except a few of four; every job asks for two cpus.  Family C — node_num at multi_k, multi_k + 1, max_upd, max_upd + 1 = lds_heap.
Family D — bursts around the task rings and the job window, more request shapes than the allocation cache has entries."""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from cranesched_amd import abi
from tests import kat

NOW = kat.NOW
GIB = 1 << 30
G = 100            # seconds between two keys of a family-A map

Case = namedtuple("Case", "name cluster jobs now running cfg condition specs nodes covers kernel")
_CACHE = {}


def raw(units):
    """raw cpu units (1/256 cpu) as the `cpu` of a kat job spec."""
    return units / 256.0


def running_of(allocs):
    """allocs: [(node, cpu_raw, end)] -> abi.Running, one job per allocation, in a fixed order that is not the order of the ends."""
    if not allocs:
        return None
    order = sorted(range(len(allocs)), key=lambda i: ((i * 37 + 11) % 101, i))
    rows = [allocs[i] for i in order]
    n = len(rows)
    z = np.zeros(n, np.uint64)
    return abi.Running(np.asarray([r[2] for r in rows], np.int64), np.arange(n + 1, dtype=np.uint32), np.asarray([r[0] for r in rows], np.uint32),
                       np.asarray([r[1] for r in rows], np.int64), np.full(n, 1 << 20, np.uint64) * np.asarray([1 if r[1] else 0 for r in rows], np.uint64),
                       z, z.copy(), z.copy())


def make(name, cluster, specs, running, cfg, condition, nodes, covers, kernel=None):
    return Case(name, cluster, kat.jobs(specs), NOW, running, cfg, condition, specs, tuple(nodes), frozenset(covers), kernel)


def placed(pl, specs, j):
    """(reason, start, sorted node list) of job j."""
    off = int(np.sum([s.get("k", 1) for s in specs[:j]]))
    k = specs[j].get("k", 1)
    nodes = sorted(int(x) for x in pl.node_idx[off:off + k] if x != abi.NODE_NONE)
    return int(pl.reason[j]), int(pl.start_sec[j]), nodes


# ---------------------------------------------------------------------------------------------------------------------------------
# family A
# ---------------------------------------------------------------------------------------------------------------------------------
class MapFrame:
    """Node 0 with a map of M entries (see the module docstring); further nodes as (cores, [(cpu_raw, end)])."""

    def __init__(self, M, cores0, others=(), zero=False, mems=None):
        self.M, self.R = M, M - 2
        self.T = cores0 * 256
        self.U, self.Y = cores0 // 4, cores0 // 8   # raw units of a running allocation | of the decisive job (Y - 1 < U: a dip lands on its entry and nowhere earlier)
        self.unit = 0 if zero else self.U
        allocs = [(0, self.unit, NOW + G * (i + 1)) for i in range(self.R)]
        cores = [cores0]
        for n, (c, al) in enumerate(others):
            cores.append(c)
            allocs += [(n + 1, cpu, end) for cpu, end in al]
        self.cluster = kat.cluster(cores, mems or [4096] * len(cores))
        self.running = running_of(allocs)

    def t(self, i):
        return NOW + G * i

    def avail(self, i):
        return self.T - (self.R - i) * self.unit

    def dip(self, e, leave):
        assert 1 <= e <= self.R - 1, "the dip's end must be the key of entry e + 1"
        return dict(cpu=raw(self.avail(e) - leave), L=G)


def followers(f):
    """What runs behind the decisive job: answers that depend on the entries its commit moved (the time maps are compared anyway)."""
    return [dict(cpu=raw(f.Y), L=G * (f.R + 1) + 70), dict(cpu=raw(3 * f.Y), L=G // 2), dict(cpu=raw(f.Y), L=G * 3)]


def a_single(name, M, cores, dips, L, want_entry, want_len, up=0, decoy=False):
    """One node; dips at the entries `dips` in front of the decisive job (Y units for L seconds), each leaving Y - 1 + up units.
    `decoy` (the twins that start now): a second node of one core that lacks one unit for the job until now + 10 and costs less than
    node 0 — a job refused now and backfilled onto the SAME node would get the same start, so a kernel that refuses node 0 wrongly
    must have somewhere else to go: the decoy, at now + 10.
    CONDITION: in front of the decisive job the map has M entries, the last dipped entry e has the key now + e * G and that many
    units; the decisive job starts on the key of entry want_entry (0: now, reason none; later: a backfill reason) on node 0 and the
    map then has want_len entries; the decoy costs less than node 0."""
    f = MapFrame(M, cores, others=[(1, [(256 - cores // 8 + 1, NOW + 10)])] if decoy else ())
    assert not decoy or want_entry == 0
    specs = [f.dip(e, f.Y - 1 + up) for e in dips] + [dict(cpu=raw(f.Y), L=L)] + followers(f)
    d = len(dips)
    spoiled = (dips[-1], f.Y - 1 + up)
    want_start = f.t(want_entry)

    def condition(ora):
        tl = ora(d).timeline(0)
        e, units = spoiled
        assert len(tl["t"]) == M and int(tl["t"][e]) == f.t(e) and int(tl["cpu_raw"][e]) == units, (name, len(tl["t"]), tl["t"][e], tl["cpu_raw"][e])
        assert int(tl["t"][-1]) == np.iinfo(np.int64).max and int(tl["cpu_raw"][-1]) == 0
        reason, start, nodes = placed(ora(d + 1).placements, specs, d)
        assert start == want_start and nodes == [0] and (reason == 0) == (want_start == NOW), (name, reason, start, nodes)
        after = len(ora(d + 1).timeline(0)["t"])
        assert after == want_len, (name, after, want_len)
        assert placed(ora().placements, specs, d) == (reason, start, nodes)
        if decoy:
            cost = ora(d).costs()
            assert cost[1] < cost[0] and int(ora(d).timeline(1)["cpu_raw"][0]) == f.Y - 1, (name, cost)
        return dict(M=M, entry=e, units=units, reason=reason, start=start - NOW, len_after=after)
    return make(name, f.cluster, specs, f.running, {}, condition, [0, 1] if decoy else [0], {"tl_chunk"})


def a_entries(shape, M):
    """The entries of a map of M entries a dip is put on: c - 1 and c where they allow one, else the last that does."""
    c = shape.tl_chunk
    es = [e for e in (c - 1, c) if e <= M - 3]
    return es or [M - 3]


def a_window_cases(shape, cores, tag):
    out = []
    c = shape.tl_chunk
    for M in (c - 1, c, c + 1, 2 * c - 1, 2 * c, 2 * c + 1):
        for e in a_entries(shape, M):
            # the window's end just past entry e (refused by it) | on its key (entry e is outside: starts now, the end key exists)
            out.append(a_single(f"win_M{M}_e{e}{tag}", M, cores, [e], G * e + 1, e + 1, M + _end_new(M, e + 1, G * e + 1)))
            out.append(a_single(f"win_M{M}_e{e}_out{tag}", M, cores, [e], G * e, 0, M, decoy=True))
            # a window over every finite key: entry e alone refuses | the same entry one unit higher (starts now, a new end key)
            long = G * (M - 1) + 50
            out.append(a_single(f"spoil_M{M}_e{e}{tag}", M, cores, [e], long, e + 1, M + 1))
            out.append(a_single(f"spoil_M{M}_e{e}_up{tag}", M, cores, [e], long, 0, M + 1, up=1, decoy=True))
    return out


def _end_new(M, start_entry, L):
    """1 when a job that starts on the key of `start_entry` and runs L seconds ends off every key of a frame's map of M entries, else 0."""
    end = G * start_entry + L
    return 0 if end % G == 0 and end // G <= M - 2 else 1


def a_run_cases(shape, cores, tag):
    """Earliest start on one node: dips at entry 1 and at entry e; the run between them lasts (e - 2) * G.  A job of exactly that
    length starts at entry 2 (a run that starts in chunk 0 and ends at entry e: c - 1, c, c + 1); one second longer and it starts
    behind entry e, in the run whose end is the map's last entry (index M - 1)."""
    out = []
    c = shape.tl_chunk
    for M in (c - 1, c, c + 1, 2 * c - 1, 2 * c, 2 * c + 1):
        es = [e for e in (c - 1, c, c + 1) if e <= M - 3] or [M - 3]
        for e in es:
            L = (e - 2) * G
            out.append(a_single(f"run_M{M}_e{e}{tag}", M, cores, [1, e], L, 2, M))
            out.append(a_single(f"run_M{M}_e{e}_long{tag}", M, cores, [1, e], L + 1, e + 1, M + _end_new(M, e + 1, L + 1)))
    return out


def a_t0_case(name, M, cores, e, dip_at, k=2):
    """Two nodes: node 1 (4 cores) is full until tB, a time inside entry e of node 0's map, so the two-node decisive job's search
    arrives at node 0 with t0 = tB.  dip_at == e: the entry covering t0 refuses, the start is the key of entry e + 1; dip_at == e - 1:
    the dip ends before tB, the job starts at tB and its commit inserts the start boundary at index e + 1 and the end boundary behind the key of entry e + 1: M + 2.
    CONDITION: in front of the decisive job node 0's map has M entries and key(e) < tB < key(e + 1); the job has a backfill reason and
    that start; behind it the map has the stated length and (second form) tB at index e + 1.  k > 2: k - 2 further free nodes of 4
    cores, the job takes all k — the same commit out of the protocols for node_num above multi_k and above max_upd."""
    f = MapFrame(M, cores, others=[(4, [(4 * 256 - 1, NOW + G * e + G // 2)])] + [(4, [])] * (k - 2))
    Y = f.Y
    tB = f.t(e) + G // 2
    specs = [f.dip(dip_at, Y - 1), dict(cpu=raw(Y), L=G, k=k)] + followers(f)
    want = f.t(e + 1) if dip_at == e else tB

    def condition(ora):
        tl = ora(1).timeline(0)
        assert len(tl["t"]) == M and int(tl["t"][e]) < tB and (e + 1 == M - 1 or tB < int(tl["t"][e + 1])) and int(tl["cpu_raw"][dip_at]) == Y - 1, name
        reason, start, nodes = placed(ora(2).placements, specs, 1)
        assert reason != 0 and start == want and nodes == list(range(k)), (name, reason, start, nodes)
        after = ora(2).timeline(0)
        if dip_at != e:
            assert len(after["t"]) == M + 2 and int(after["t"][e + 1]) == tB and int(after["t"][e + 2]) == f.t(e + 1) and int(after["t"][e + 3]) == tB + G, (name, len(after["t"]))
        return dict(M=M, covering_entry=e, tB=tB - NOW, reason=reason, start=start - NOW, len_after=len(after["t"]))
    return make(name, f.cluster, specs, f.running, {}, condition, range(k), {"tl_chunk"})


def a_t0_cases(shape, cores, tag):
    out = []
    c = shape.tl_chunk
    for M in (c - 1, c, c + 1, 2 * c - 1, 2 * c, 2 * c + 1):
        es = [e for e in (c - 2, c - 1, c) if e <= M - 3] or [M - 3]
        for e in es:
            out.append(a_t0_case(f"t0_M{M}_e{e}{tag}", M, cores, e, e))
            out.append(a_t0_case(f"t0_M{M}_e{e}_free{tag}", M, cores, e, e - 1))
            for k in (shape.multi_k + 1, shape.lds_heap):   # the same commit from the sequential multi-node protocol and from the general path
                out.append(a_t0_case(f"t0_M{M}_e{e}_free_k{k}{tag}", M, cores, e, e - 1, k))
    return out


def a_excl_case(name, M, cores, e, inside):
    """Exclusive job (every entry inside its window must hold the whole node).  Node 0's R running allocations hold NOTHING: M keys,
    every finite entry the whole node.  Node 1 (4 cores) is full until key(e); the two-node job in front (8 GiB a node: node 2 has 4)
    therefore starts at key(e), for G seconds: entry e of node 0 — and only it — is short.  Node 2 (4 cores) lends one raw cpu unit
    until now + 10: the cheapest node of the three, not free now.  The exclusive job's window ends on key(e) (starts now on node 0,
    the second node in cost order) or one second past it (`inside`: refused on all three, backfilled onto the cheapest, node 2, at
    now + 10).  A kernel that takes entry e for inside the first window gives the second answer, one that leaves it out of the second
    window the first.  CONDITION: in front of the exclusive job node 0's map has M entries, all finite ones but entry e equal to the
    node's total; node 2 costs less than node 0 and node 0 less than node 1; the start, node and reason as stated."""
    f = MapFrame(M, cores, others=[(4, [(4 * 256 - 1, NOW + G * e)]), (4, [(1, NOW + 10)])], zero=True, mems=[4096, 4096, 4])
    specs = [dict(cpu=raw(f.Y), L=G, k=2, mem_gib=8), dict(cpu=1, L=G * e + (1 if inside else 0), excl=1), dict(cpu=raw(f.Y), L=G * 3), dict(cpu=1, L=G * (e + 2))]

    def condition(ora):
        tl = ora(1).timeline(0)
        short = [i for i in range(M - 1) if int(tl["cpu_raw"][i]) != f.T]
        assert len(tl["t"]) == M and short == [e] and int(tl["t"][e]) == f.t(e), (name, len(tl["t"]), short)
        assert placed(ora(1).placements, specs, 0)[1:] == (f.t(e), [0, 1]), name
        cost = ora(1).costs()
        assert cost[2] < cost[0] < cost[1], (name, cost)
        reason, start, nodes = placed(ora(2).placements, specs, 1)
        if inside:
            assert reason != 0 and start == NOW + 10 and nodes == [2], (name, reason, start, nodes)
        else:
            assert reason == 0 and start == NOW and nodes == [0], (name, reason, start, nodes)
        return dict(M=M, spoiling_entry=e, costs=[float(x) for x in cost], reason=reason, start=start - NOW, nodes=nodes)
    return make(name, f.cluster, specs, f.running, {}, condition, [0, 1, 2], {"tl_chunk"})


def a_excl_cases(shape, cores, tag):
    out = []
    c = shape.tl_chunk
    for M in (c - 1, c, c + 1, 2 * c - 1, 2 * c, 2 * c + 1):
        for e in a_entries(shape, M):
            out.append(a_excl_case(f"excl_M{M}_e{e}{tag}", M, cores, e, True))
            out.append(a_excl_case(f"excl_M{M}_e{e}_out{tag}", M, cores, e, False))
    return out


def a_cap_case(name, M, cores, limit, covers):
    """kAlgoMaxJobNumPerNode (:6194): one node whose map has M entries, the limit `limit` (0: the default 1000).  CONDITION: M >= limit —
    no job is placed and the map stays; M == limit - 1 — the first job starts now and adds an end key, the second finds no node."""
    f = MapFrame(M, cores)
    specs = [dict(cpu=raw(f.Y), L=G // 2), dict(cpu=raw(f.Y), L=G // 2 + 10)]
    eff = limit or 1000

    def condition(ora):
        assert len(ora(0).timeline(0)["t"]) == M
        a, b = placed(ora().placements, specs, 0), placed(ora().placements, specs, 1)
        after = len(ora().timeline(0)["t"])
        if M >= eff:
            assert a == (abi.REASON_RESOURCE, 0, []) and b == a and after == M, (name, a, b, after)
        else:
            assert M == eff - 1 and a == (0, NOW, [0]) and b == (abi.REASON_RESOURCE, 0, []) and after == M + 1, (name, a, b, after)
        return dict(M=M, limit=eff, first=a[:2], second=b[:2], len_after=after)
    return make(name, f.cluster, specs, f.running, dict(max_job_num_per_node=limit) if limit else {}, condition, [0], covers)


def a_cap_cases(shape, cores, tag):
    c = shape.tl_chunk
    out = [a_cap_case("cap_default_at" + tag, 1000, cores, 0, {"tl_chunk"}), a_cap_case("cap_default_below" + tag, 999, cores, 0, {"tl_chunk"})]
    for lim in (c, c + 1):
        out += [a_cap_case(f"cap_cfg{lim}_at{tag}", lim, cores, lim, {"tl_chunk"}), a_cap_case(f"cap_cfg{lim}_below{tag}", lim - 1, cores, lim, {"tl_chunk"})]
    # the longest map a snapshot may bring and the highest limit a handle takes (limit + 2 <= tl_cap): passed over by the default limit and by
    # that one; one entry below it the commit takes the map to tl_cap - 2 entries and the node is passed over from then on
    top = shape.tl_cap - 2
    out += [a_cap_case("cap_tlcap_default" + tag, top, cores, 0, {"tl_cap"}), a_cap_case("cap_tlcap_at" + tag, top, cores, top, {"tl_cap"}),
            a_cap_case("cap_tlcap_below" + tag, top - 1, cores, top, {"tl_cap"})]
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# family B
# ---------------------------------------------------------------------------------------------------------------------------------
def b_cluster(N, big, mem_gib):
    """N nodes of one core and 16 GiB, the nodes of `big` with four cores and mem_gib[i] (built with numpy: up to 65 537 nodes)."""
    cores = np.ones(N, np.int64)
    mem = np.full(N, 16, np.uint64)
    for n, m in zip(big, mem_gib):
        cores[n] = 4
        mem[n] = m
    lo = ((np.uint64(1) << cores.astype(np.uint64)) - np.uint64(1)).astype(np.uint64)
    z = np.zeros(N, np.uint64)
    return abi.Cluster(cores * 256, mem * np.uint64(GIB), lo, z, z.copy(), np.asarray([0, N], np.uint32), np.arange(N, dtype=np.uint32))


def b_one_case(name, N, lanes, covers, kernel):
    """One-node jobs of two cpus on a partition where only a few nodes have more than one core.  The groups, in the queue's order: the
    partition's last node; the first node of its last tile row; 63 | 64 (a wave's edge); lanes - 1 | lanes (a row's edge).  Memory tells
    them apart: the r-th group's jobs ask for what only its own nodes and the groups before it have, and those are taken.  Phase 1:
    one job per node, group by group — a group of two has two nodes of equal cost and the lower index goes first, then the higher one is
    the only node left.  Phase 2: a four-cpu job per node, backfilled behind phase 1 in cost-and-index order.  Phase 3: two-cpu jobs
    whose windows end around that reservation (L = 150, 101, 100, 116, 96, then 100s): refused by it or not, second by second.
    CONDITION: the phase-1 jobs start now on exactly the stated nodes in the stated order; phase 2 is backfilled to now + 100 on every
    one of them once; phase 3 holds jobs that start now and jobs that do not."""
    last_row = lanes * ((N - 1) // lanes)
    groups, seen = [], set()
    for g in ([N - 1], [last_row], [63, 64], [lanes - 1, lanes]):
        g = [n for n in g if 0 <= n < N and n not in seen]
        seen.update(g)
        if g:
            groups.append(sorted(g))
    order = [n for g in groups for n in g]                      # the nodes in the order phase 1 takes them
    nb = len(order)
    rank, r = {}, nb
    for g in groups:                                            # earlier groups rank higher; inside a group the higher index does
        for n in g:
            r -= 1
        for i, n in enumerate(g):
            rank[n] = r + i
    big = sorted(order)
    cluster = b_cluster(N, big, [256 + 16 * rank[n] + 8 for n in big])
    specs = []
    for g in groups:
        specs += [dict(cpu=2, L=100, mem_gib=256 + 16 * rank[g[0]]) for _ in g]
    specs += [dict(cpu=4, L=100) for _ in big]
    tail = [150, 101, 100, 116, 96] + [100] * (nb - 1)
    specs += [dict(cpu=2, L=L) for L in tail]

    def condition(ora):
        pl = ora().placements
        p1 = [placed(pl, specs, j) for j in range(nb)]
        assert p1 == [(0, NOW, [n]) for n in order], (name, p1, order)
        p2 = [placed(pl, specs, nb + j) for j in range(nb)]
        assert all(r != 0 and s == NOW + 100 for r, s, _ in p2) and sorted(n[0] for _, _, n in p2) == big, (name, p2)
        p3 = [placed(pl, specs, 2 * nb + j) for j in range(len(tail))]
        now3 = sum(1 for r, s, _ in p3 if r == 0)
        assert 0 < now3 < len(p3) and p3[0][0] != 0 and p3[1][0] != 0 and p3[2][0] == 0, (name, p3)
        return dict(N=N, lanes=lanes, phase1=order, phase2=[n[0] for _, _, n in p2], phase3_now=now3, phase3=len(p3))
    return make(name, cluster, specs, None, {}, condition, big, covers, kernel)


def b_multi_case(name, N, k8, covers, kernel):
    """node_num 2 and k8 = pipe_max_k (two cpus per node) on a partition whose four-core nodes are 56 .. 63, 64 and one node in each of
    the waves behind (64 * i + 7, i = 2 ..).  CONDITION: the k8-node job takes 56 .. 63 — one wave's lanes, its k-th and (k + 1)-th
    candidates 63 | 64 of equal cost on either side of the wave's edge; the two-node job behind it takes 64 and the next wave's node;
    the second k8-node job takes one node per wave where the partition has that many."""
    first = list(range(64 - k8, 64))
    spread = [64 * i + 7 for i in range(2, 3 + k8) if 64 * i + 7 < N]
    big = first + ([64] if N > 64 else []) + spread
    cluster = b_cluster(N, big, [16] * len(big))
    specs = [dict(cpu=2, L=100, k=k8), dict(cpu=2, L=100, k=2), dict(cpu=2, L=100, k=k8), dict(cpu=2, L=100, k=2), dict(cpu=2, L=60, k=k8)]
    specs += [dict(cpu=2, L=50) for _ in range(6)] + [dict(cpu=4, L=30, k=2)]

    def condition(ora):
        pl = ora().placements
        j0, j1, j2 = (placed(pl, specs, j) for j in range(3))
        assert j0 == (0, NOW, first), (name, j0)
        if len(spread) >= 1:
            assert j1 == (0, NOW, [64, spread[0]]), (name, j1)
        if len(spread) >= 1 + k8:
            assert j2 == (0, NOW, spread[1:1 + k8]) and len({n // 64 for n in j2[2]}) == k8, (name, j2)
        return dict(N=N, first=j0[2], second=j1[2], third=j2[2], rest=[placed(pl, specs, j)[:2] for j in range(3, len(specs))])
    return make(name, cluster, specs, None, {}, condition, big, covers, kernel)


def b_tiny_case(N):
    """A partition of N = 1, 2, 3 nodes of four cores: two-cpu jobs until it is full and past that, a job over all N nodes, one over
    N + 1.  CONDITION: the first 2 N jobs start now, node by node; the next is backfilled; the N + 1-node job finds no nodes."""
    cluster = kat.cluster([4] * N, [16] * N)
    specs = [dict(cpu=2, L=100 + 10 * i) for i in range(2 * N + 1)] + [dict(cpu=1, L=50, k=N), dict(cpu=1, L=50, k=N + 1)]

    def condition(ora):
        pl = ora().placements
        p = [placed(pl, specs, j) for j in range(len(specs))]
        assert all(x[0] == 0 and x[1] == NOW for x in p[:2 * N]) and p[2 * N][0] != 0 and p[2 * N][1] > NOW, (N, p)
        assert p[-2][2] == list(range(N)) and p[-1] == (abi.REASON_RESOURCE, 0, []), (N, p)
        return dict(N=N, nodes=[x[2] for x in p], starts=[x[1] - NOW for x in p])
    return make(f"tiny_n{N}", cluster, specs, None, {}, condition, range(N), {"select", "pipe", "wide"})


FAMILY_WORD = {"select": "legacy", "pipe": "pipe", 64: "wide", 32: "wide32", 16: "wide16", 8: "wide8"}


def serving_kernel(shape, family, N):
    """What last_kernel() must name for ONE partition of N nodes under the family's CNS_SELECT_KERNEL word (csrc/plan_host.inc, held to
    these rules by tests/cpp/plan_host_test.cpp): ("prefix", "suffix") of the name, or None where nothing serves (legacy past k_select's
    widest tile: CNS_ERR_UNSUPPORTED)."""
    width = lambda t: next((w for w in t.widths if N <= t.lanes * w), 0)
    widest = shape.wide[0][1]
    if N > widest.lanes * widest.widths[-1]:
        return ("k_", "slots")                                   # k_giant, or k_mem where its helpers cannot run: both name the group's slots
    if family not in ("select", "pipe"):
        for waves, t in shape.wide:
            if waves <= family and width(t):
                return (f"k_wide<{width(t)}>", f"x{waves}")
    if family != "select" and width(shape.pipe):
        return (f"k_pipe<{width(shape.pipe)}>", "")
    if width(shape.select):
        return (f"k_select<{width(shape.select)}>", "")
    return None


def b_cases(shape):
    out = []
    fams = [("select", shape.select, "select"), ("pipe", shape.pipe, "pipe")] + [(waves, t, "wide") for waves, t in shape.wide]
    for fam, tiles, field in fams:
        tag = fam if isinstance(fam, str) else f"wide{fam}"
        for w in tiles.widths:
            for N in (tiles.lanes * w - 1, tiles.lanes * w, tiles.lanes * w + 1):
                kern = (FAMILY_WORD[fam], serving_kernel(shape, fam, N))
                covers = {field} | ({"sel_dip_max_npl"} if fam == "select" and w in _dip_widths(shape) else set())
                out.append(Lazy(f"one_{tag}_w{w}_n{N}", b_one_case, (N, tiles.lanes, covers, kern)))
                out.append(Lazy(f"multi_{tag}_w{w}_n{N}", b_multi_case, (N, shape.pipe_max_k, covers | {"pipe_max_k"}, kern)))
    return out


class Lazy:
    """A family-B case by name: its cluster (up to 65 537 nodes) is built when the case is asked for and not kept."""

    def __init__(self, name, fn, args):
        self.name, self.fn, self.args, self.covers = name, fn, args, frozenset(args[2])

    def build(self):
        return self.fn(self.name, *self.args)


def _dip_widths(shape):
    """k_select's widest tile that keeps a dip per node and the next wider one."""
    ws = shape.select.widths
    keep = [w for w in ws if w <= shape.sel_dip_max_npl]
    nxt = [w for w in ws if w > shape.sel_dip_max_npl]
    return set(keep[-1:] + nxt[:1])


# ---------------------------------------------------------------------------------------------------------------------------------
# family C
# ---------------------------------------------------------------------------------------------------------------------------------
def c_case(shape, k, kind, covers):
    """A job of node_num k on a partition of k + 3 nodes of 8 cores, followed by 2 k + 6 one-node jobs of one cpu (four behind an exclusive job) and 1000 s: each goes
    to the cheapest node that fits, so their order walks the k nodes just committed by cost — a lost cost or front update for one of
    them changes an answer.  kind: now (starts now, ntasks == k) | nt (starts now, ntasks == k + 2, up to two tasks a node) | excl
    (exclusive) | bf, ntbf (every node holds 7 cpus until now + 100 + 10 * index: backfilled to the k-th node's end).
    CONDITION: the job has reason none and start now, or a backfill reason and start now + 100 + 10 * (k - 1); it is placed on nodes
    0 .. k - 1; the followers land on every node of the partition."""
    n = k + 3
    busy = kind in ("bf", "ntbf")
    cluster = kat.cluster([8] * n, [64] * n)
    run = running_of([(i, 7 * 256 - 1, NOW + 100 + 10 * i) for i in range(n)]) if busy else None
    job = dict(cpu=2, L=100, k=k)
    if kind in ("nt", "ntbf"):
        job.update(cpu=1 if kind == "nt" else 2, ntasks=k + 2, tmin=1, tmax=2)
    if kind == "excl":
        job.update(cpu=1, excl=1)
    specs = [job] + [dict(cpu=4 if kind == "excl" else 1, L=1000) for _ in range(2 * k + 6)]   # (excl: the three spare nodes hold six, the rest wait for the job's nodes)
    want = NOW + 100 + 10 * (k - 1) if busy else NOW

    def condition(ora):
        pl = ora().placements
        reason, start, nodes = placed(pl, specs, 0)
        assert (reason == 0) == (not busy) and start == want and nodes == list(range(k)), (k, kind, reason, start, nodes)
        f = [placed(pl, specs, j) for j in range(1, len(specs))]
        visited = sorted({x[2][0] for x in f if x[2]})
        assert visited == list(range(n)), (k, kind, visited)
        return dict(k=k, kind=kind, reason=reason, start=start - NOW, followers=[x[2][0] if x[2] else None for x in f])
    return make(f"k{k}_{kind}", cluster, specs, run, {}, condition, range(n), covers)


def c_cases(shape):
    out = []
    ks = [(shape.multi_k, {"multi_k", "pipe_max_k"}), (shape.multi_k + 1, {"multi_k", "pipe_max_k"}), (shape.max_upd, {"max_upd"}),
          (shape.max_upd + 1, {"max_upd", "lds_heap"})]
    if shape.pipe_max_k != shape.multi_k:
        ks += [(shape.pipe_max_k, {"pipe_max_k"}), (shape.pipe_max_k + 1, {"pipe_max_k"})]
    if shape.lds_heap != shape.max_upd + 1:
        ks += [(shape.lds_heap - 1, {"lds_heap"}), (shape.lds_heap, {"lds_heap"})]
    for k, cov in ks:
        for kind in ("now", "bf", "nt", "ntbf", "excl"):
            out.append(c_case(shape, k, kind, cov))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# family D
# ---------------------------------------------------------------------------------------------------------------------------------
def d_burst_case(name, n, nodes, mid, covers):
    """n consecutive one-node jobs of a quarter cpu and equal length that start now, on `nodes` equal nodes of 64 cores (one node:
    every task depends on the one before it); `mid`: the job in the middle asks for a whole node and must wait for the others' end.
    CONDITION: every job but that one has reason none and start now; that one a backfill reason and start now + 100."""
    cluster = kat.cluster([64] * nodes, [512] * nodes)
    specs = [dict(cpu=0.25, L=100) for _ in range(n)]
    if mid:
        specs[n // 2] = dict(cpu=64, L=100)

    def condition(ora):
        pl = ora().placements
        p = [placed(pl, specs, j) for j in range(n)]
        for j, (reason, start, nd) in enumerate(p):
            if mid and j == n // 2:
                assert reason != 0 and start == NOW + 100, (name, j, reason, start)
            else:
                assert reason == 0 and start == NOW, (name, j, reason, start)
        return dict(jobs=n, nodes=nodes, on_node0=sum(1 for x in p if x[2] == [0]), mid=p[n // 2][:2] if mid else None)
    return make(name, cluster, specs, None, {}, condition, range(nodes), covers)


def d_burst_cases(shape):
    out, done = [], set()
    rings = [("pipe_xring", shape.pipe_xring), ("pipe_ring", shape.pipe_ring), ("wide_task_ring", shape.wide_task_ring), ("wide_window", shape.wide_window)]
    for r in sorted({v for _, v in rings if v}):
        cov = {f for f, v in rings if v == r}
        for n in (r - 1, r, r + 1, 2 * r + 1):
            for nodes, mid in ((1, False), (2, False), (1, True), (2, True)):
                name = f"burst_{n}_on{nodes}" + ("_mid" if mid else "")
                if name not in done and n >= 3:
                    done.add(name)
                    out.append(d_burst_case(name, n, nodes, mid, cov))
    return out


def d_cache_case(shape):
    """More request shapes than the allocation cache has entries, on one node type: 16 nodes of 256 cores and 8 GRES slots that hold
    all but half a cpu until now + 100, so every job is backfilled — the path that consults the cache.  The shapes: 1 .. alloc_cache - 6
    whole cpus without GRES (their allocations against res_total differ in the core ids: an entry answered for another shape shows),
    and 1 .. 4 cpus with a GRES total of 1 .. 7.  The whole list comes twice, the second time in another order and with twice the
    memory: equal shape, different memory.  No knowledge of the hash: with more shapes than entries some share one.
    CONDITION: more than alloc_cache distinct (cpu, GRES total) pairs, all but 28 of them with the same GRES total; every job is
    backfilled (a reason, a start after now)."""
    nodes = 16
    lay = abi.GresLayout(class_name=[0], class_shift=[0], class_width=[8])
    cluster = kat.cluster([256] * nodes, [4096] * nodes, gres=[0xFF] * nodes, layout=lay)
    run = running_of([(i, 256 * 256 - 128, NOW + 100) for i in range(nodes)])
    shapes = [(c, 0) for c in range(1, shape.alloc_cache - 5)] + [(c, g) for c in range(1, 5) for g in range(1, 8)]
    spec = lambda c, g, mem: dict(cpu=c, L=40 + 3 * g + c % 7, mem_gib=mem, **({"gtot": [g]} if g else {}))
    second = sorted(range(len(shapes)), key=lambda i: ((i * 53 + 7) % 89, i))
    specs = [spec(c, g, 1) for c, g in shapes] + [spec(*shapes[i], 2) for i in second]

    def condition(ora):
        pl = ora().placements
        assert len(set(shapes)) > shape.alloc_cache and sum(1 for _, g in shapes if g) == 28
        p = [placed(pl, specs, j) for j in range(len(specs))]
        assert all(r != 0 and s > NOW and len(nd) == 1 for r, s, nd in p), [x for x in p if x[0] == 0 or not x[2]][:3]
        longest = max(len(ora().timeline(n)["t"]) for n in range(nodes))
        return dict(shapes=len(set(shapes)), jobs=len(specs), last_start=max(s for _, s, _ in p) - NOW, nodes_used=len({x[2][0] for x in p}), longest_map=longest)
    return make("cache_shapes", cluster, specs, run, {}, condition, range(nodes), {"alloc_cache"})


# ---------------------------------------------------------------------------------------------------------------------------------
def family_a(shape):
    """Every case twice: on a node of 256 cores (core ids above 127: the kernels' four-word instantiations) and, names ending in _c64,
    on one of 64 (the two-word ones, which serve every cluster without such nodes)."""
    out = []
    for cores, tag in ((256, ""), (64, "_c64")):
        out += a_window_cases(shape, cores, tag) + a_run_cases(shape, cores, tag) + a_t0_cases(shape, cores, tag) + a_excl_cases(shape, cores, tag) + a_cap_cases(shape, cores, tag)
    return out


def family_b(shape):
    return b_cases(shape)


def family_c(shape):
    return c_cases(shape)


def family_d(shape):
    return d_burst_cases(shape) + [d_cache_case(shape)] + [b_tiny_case(n) for n in (1, 2, 3)]


FAMILIES = {"A": family_a, "B": family_b, "C": family_c, "D": family_d}


def cases(shape, family):
    """The cases of a family for that shape, built once per process: {name: Case} in a fixed order."""
    key = (shape, family)
    if key not in _CACHE:
        lst = FAMILIES[family](shape)
        assert len({c.name for c in lst}) == len(lst), "case names repeat"
        _CACHE[key] = {c.name: c for c in lst}
    return _CACHE[key]


def case_names(shape, family):
    return list(cases(shape, family))


def case(shape, family, name):
    c = cases(shape, family)[name]
    return c.build() if isinstance(c, Lazy) else c


# The shipped shape (tests/test_select_abi.py pins it): the lists pytest parametrizes over are built for it at import, without the library.
SHIPPED = abi.SelectShape(64, 1008, 8, 8, 32, 33, 256, 32, 64, 8, 32, 19, abi.TileShape(448, (1, 3, 10, 19, 28, 37)), abi.TileShape(512, (1, 4, 8, 16)),
                          ((64, abi.TileShape(4096, (1, 2, 4, 8, 16))), (32, abi.TileShape(2048, (1, 2, 4, 8))), (16, abi.TileShape(1024, (1, 2, 4, 8))),
                           (8, abi.TileShape(512, (1, 2, 4, 8)))))
