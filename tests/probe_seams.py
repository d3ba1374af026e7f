"""Cases on the seams of the what-if probes (csrc/probe_kernel.inc, probe_host.inc), every size taken from cns_probe_shape
(engine.probe_shape()) and cns_select_shape.  No HIP in here and no random numbers.  Expected values never come from this file:
tests/test_probe_seams.py computes tests/probe_case.expected (one oracle cycle over queue + [probe]) for every case and asserts its
CONDITION — a function of the oracle's answers that states what puts the case on its seam; tests/test_gpu_probe_seams.py holds the
engine to the same expected answers.

A case is a PCase: the snapshot (cluster, running, reservations, cfg), the cycle's `queue`, the probe table `probes`, and
  condition(ctx)  ctx.exp: the expected Placements of the probes; ctx.cycle: the oracle's run of the queue (costs, final time maps);
                  ctx.answer(i): (reason, start, nodes, ntasks) of probe i; ctx.select_ora(case): the runner a select case's own
                  CONDITION takes (family R).  Returns a dict of what it saw.
  nodes           the seam nodes: their time maps must be unchanged behind the probes
  covers          the fields of probe_shape() the case stands on
  kernel          family R-B: (CNS_SELECT_KERNEL word, what last_kernel() must name)
  before          family U: the queue of an earlier cycle on the same handle (its state must not show)
  one_sided       why the table cannot hold both a probe that starts now and one that does not (None: it holds both)
  dip             families D, U: (part-slot, seconds, who posts it) — the dip that must stand in KParams::dip_* before the probes run
  plan            family K: [(CNS_PROBE_SCRATCH_CAP in bytes or None, the grid cns_debug_get_probe_plan must report or None, the stride)]

Families.  R — prefix replay of tests/select_seams.py (the cases are reused, not copied): a probe of job n behind the cycle over jobs
0 .. n - 1 gets what the oracle's whole-queue run wrote for job n.  Split `d`: the cycle in front of the decisive job, that job as the
probe; split `f`: the cycle up to and including it, every job behind it as an independent probe (the first of them is job d + 1 of the
whole queue).  Where a prefix is empty the cycle runs over one job that no node's total fits (nothing is committed), as the select
suite does.  S — the slot walk in strides of `block`.  K — node_num against the 64-lane loops, the heap and the scratch plan.
T — 64 node types.  D — dips behind k_select.  U — state no selection kernel wrote.  V — reservations.
What the cases are built around:
  * R-D: every job of cache_shapes and of tiny_n1..3 is a probe behind its own prefix; of a burst, the last job.
  * R-B: one node past k_select's widest tile the cycle is refused under `legacy` (the select suite asserts the refusal); the replay
    of that tile takes the partition that fills it.
  * K: a probe of node_num == n_p cannot evict from its heap (there is no (k + 1)-th candidate) and one of n_p + 1 finds no nodes
    whatever it asks: their ntasks > node_num twins have the early break at the last candidate / are answered "Resource".
  * S, walk-continues: the future entry below the request comes from a reservation (a queue job would change the node's cost and take
    the walk off the tie; the engine takes no reservation without cpus); the next candidate carries reservations of the same cpu
    share and length, so both cost the same; an earlier, harmless reservation entry takes the node's one dip, so that the candidate
    passes the filters and falls to the exact test.
  * D: k_select and k_pipe keep the dips they find in registers and LDS (select_kernels.hip: post_dip) and never store them to
    KParams::dip_*; what a probe reads there comes from k_init_nodes (a pending reservation's dip) and from k_wide (record_dip).
    Every dip case therefore comes twice: `dip_*`, a backfilled queue job leaves the entry (the dip is in the array behind k_wide
    only, and not even there where the refusal is by a name's total alone: those two cases are plain parity), and `rdip_*`, the same
    entry left by a reservation — the dip k_init_nodes posts, which cns_debug_get_dips must show under every kernel."""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from cranesched_amd import abi
from tests import kat
from tests import select_seams as ss

NOW = kat.NOW
GIB = 1 << 30
INF = np.iinfo(np.int64).max
NO_NODE_FITS = [dict(cpu=100000, L=1)]   # the queue of an empty prefix: one job no node's total fits, nothing is committed

PCase = namedtuple("PCase", "name cluster queue probes now running reservations cfg condition nodes covers kernel before one_sided dip plan")
_CACHE = {}
_SELECT_SEEN = {}

# The shipped shapes (tests/test_probe_abi.py pins this one, tests/test_select_abi.py the other): the lists pytest parametrizes over
# are built for them at import, without the library.
SHIPPED = abi.ProbeShape(64, 0xFFFF, 0xFFFF, 15, 8, 4, 64, 80, 0xFFFFFFFF, 1 << 30)
SEL = ss.SHIPPED


def pjobs(specs):
    """kat.jobs and, per spec: `mem` (bytes per task, instead of mem_gib), `cpu_raw` (1/256 cpus per task, instead of cpu), `resv`
    (the reservation the job is submitted into)."""
    j = kat.jobs(specs)
    for i, s in enumerate(specs):
        if "mem" in s:
            j.task_mem[i] = np.uint64(s["mem"])
        if "cpu_raw" in s:
            j.task_cpu_raw[i] = s["cpu_raw"]
    if any("resv" in s for s in specs):
        j.reservation = np.asarray([s.get("resv", abi.RESV_NONE) for s in specs], np.uint32)
    return j


def make(name, cluster, queue, probes, condition, nodes, covers, running=None, reservations=None, cfg=None, kernel=None, before=None,
         one_sided=None, dip=None, plan=None, now=NOW):
    q = queue if isinstance(queue, abi.Jobs) else pjobs(queue)
    p = probes if isinstance(probes, abi.Jobs) else pjobs(probes)
    b = before if before is None or isinstance(before, abi.Jobs) else pjobs(before)
    return PCase(name, cluster, q, p, now, running, reservations, cfg or {}, condition, tuple(int(n) for n in nodes), frozenset(covers), kernel, b,
                 one_sided, dip, tuple(plan or ()))


def answer(exp, probes, i):
    """(reason, start, sorted node list, ntasks per node in that order) of probe i."""
    off = int(np.sum(probes.node_num[:i]))
    k = int(probes.node_num[i])
    rec = sorted((int(exp.node_idx[o]), int(exp.ntasks[o])) for o in range(off, off + k) if exp.node_idx[o] != abi.NODE_NONE)
    return int(exp.reason[i]), int(exp.start_sec[i]), [n for n, _ in rec], [t for _, t in rec]


def bits(costs):
    return [int(x) for x in np.asarray(costs, np.float64).view(np.uint64)]


def idle(n, cores=1, mem=16):
    return kat.cluster([cores] * n, [mem] * n)


def starts_now(a):
    return a[0] == 0 and a[1] == NOW


# ---------------------------------------------------------------------------------------------------------------------------------
# family R: prefix replay of the selection seams
# ---------------------------------------------------------------------------------------------------------------------------------
def decisive(fam, sc):
    """The index of the job a select case is about."""
    if fam == "C":
        return 0
    if sc.name.startswith("excl_"):
        return 1
    if sc.name.startswith("cap_"):
        return 0
    return len(sc.specs) - 4          # win_, spoil_, run_, t0_: the job in front of the three followers


def replay(name, fam, sc, n, idx, covers, kernel=None):
    """The cycle over specs[:n] of select case `sc`, the jobs `idx` of it as independent probes.
    CONDITION: the select case's own CONDITION, called as it is; the expected answer of a probe of job n is what the oracle's run of the
    whole queue wrote for job n."""
    specs = sc.specs
    probes = [specs[i] for i in idx]

    def condition(ctx):
        ora = ctx.select_ora(sc)
        key = (fam, sc.name, ctx.backend)
        if key not in _SELECT_SEEN:       # (once per select case and backend: its replays share it)
            _SELECT_SEEN[key] = sc.condition(ora)
        seen = _SELECT_SEEN[key]
        tied = 0
        for q, i in enumerate(idx):
            if i == n:                # the job directly behind the prefix: the ordered loop is sequential
                r, s, nodes = ss.placed(ora().placements, specs, i)
                a = ctx.answer(q)
                assert (a[0], a[1], a[2]) == (r, s, nodes), (name, i, a, (r, s, nodes))
                whole = ora().placements
                o = int(np.sum([x.get("k", 1) for x in specs[:i]]))
                po = int(np.sum(ctx.probes.node_num[:q]))
                for f in ("node_idx", "ntasks", "cpu_raw", "mem", "core_lo", "core_hi", "core_w2", "core_w3", "gres"):
                    k = specs[i].get("k", 1)
                    assert np.array_equal(getattr(whole, f)[o:o + k], getattr(ctx.exp, f)[po:po + k]), (name, i, f)
                tied += 1
        assert tied == 1, name
        return dict(select=seen, prefix=n, probes=list(idx), answers=[ctx.answer(q)[:2] for q in range(len(idx))])
    return make(name, sc.cluster, specs[:n] or NO_NODE_FITS, probes, condition, sc.nodes, covers, running=sc.running, cfg=sc.cfg, kernel=kernel,
                one_sided="the jobs of a select case: one probe, or whatever the commit in front of the followers leaves them")


class LazyCase:
    def __init__(self, name, fn):
        self.name, self.fn = name, fn

    def build(self):
        return self.fn()


def r_two_splits(fam, covers):
    out = []
    for sname, sc in ss.cases(SEL, fam).items():
        d = decisive(fam, sc)
        out.append(LazyCase(f"{sname}__d", lambda sc=sc, d=d, sname=sname: replay(f"{sname}__d", fam, sc, d, [d], covers)))
        if d + 1 < len(sc.specs):
            out.append(LazyCase(f"{sname}__f", lambda sc=sc, d=d, sname=sname: replay(f"{sname}__f", fam, sc, d + 1, list(range(d + 1, len(sc.specs))), covers)))
    return out


def family_ra(shape):
    return r_two_splits("A", {"block"})


def family_rc(shape):
    return r_two_splits("C", {"block", "heap_ent_bytes"})


def family_rd(shape):
    out = []
    for sname, sc in ss.cases(SEL, "D").items():
        J = len(sc.specs)
        if sname.startswith("tiny_n") or sname == "cache_shapes":
            at = list(range(J))
        else:
            at = [J - 1]
        for n in at:
            out.append(LazyCase(f"{sname}__j{n}", lambda sc=sc, n=n, sname=sname: replay(f"{sname}__j{n}", "D", sc, n, [n], {"block"})))
    return out


def family_rb(shape):
    """Per kernel family the lanes * w + 1 cases of the narrowest and the widest tile; the last job is the probe."""
    out = []
    fams = [("select", SEL.select), ("pipe", SEL.pipe)] + [(waves, t) for waves, t in SEL.wide]
    lazies = ss.cases(SEL, "B")
    for fam, tiles in fams:
        tag = fam if isinstance(fam, str) else f"wide{fam}"
        for w in (tiles.widths[0], tiles.widths[-1]):
            N = tiles.lanes * w + 1
            if ss.serving_kernel(SEL, fam, N) is None:       # (one node past k_select's widest tile under `legacy`: the cycle is refused)
                N -= 1
            for kind in ("one", "multi"):
                sname = f"{kind}_{tag}_w{w}_n{N}"
                lz = lazies[sname]

                def build(lz=lz, sname=sname):
                    sc = lz.build()
                    n = len(sc.specs) - 1
                    return replay(f"{sname}__last", "B", sc, n, [n], {"block"}, kernel=sc.kernel)
                out.append(LazyCase(f"{sname}__last", build))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# family S: the slot walk
# ---------------------------------------------------------------------------------------------------------------------------------
def s_cluster(N, big):
    """N nodes of one core and 16 GiB, the nodes of `big` with 64 GiB: every cost is 0.0, memory alone tells the nodes apart."""
    mem = [16] * N
    for n in big:
        mem[n] = 64
    return kat.cluster([1] * N, mem)


S_PROBES = [dict(cpu=1, L=100, mem_gib=20), dict(cpu=1, L=100, mem_gib=1), dict(cpu=1, L=100, mem_gib=100)]


def s_only(shape, N, s):
    """The only node that fits the first probe sits at slot s.  CONDITION: every cost is the same bit pattern; the oracle starts the
    probe now on node s, the small probe now on node 0 (the tie on the lowest index), and finds no node for the third."""
    def condition(ctx):
        c = bits(ctx.cycle.costs())
        assert len(set(c)) == 1 and len(c) == N, c[:4]
        a, b, z = ctx.answer(0), ctx.answer(1), ctx.answer(2)
        assert starts_now(a) and a[2] == [s] and starts_now(b) and b[2] == [0] and z[:3] == (abi.REASON_RESOURCE, 0, []), (N, s, a, b, z)
        return dict(N=N, slot=s, cost_bits=c[0])
    return make(f"only_n{N}_s{s}", s_cluster(N, [s]), NO_NODE_FITS, S_PROBES, condition, [s, 0], {"block"})


def s_pair(shape, N, lo, hi, what):
    """Two nodes fit the first probe, at slots lo < hi, of equal cost.  what == "lane": hi = lo + block, one lane sees both and must
    keep the smaller; "wave": they sit in different lanes and hi's lane is the lower one (70 and 6), so the wave reduction must break
    the tie on the slot.  CONDITION: the costs are the same bit pattern and the oracle picks lo."""
    def condition(ctx):
        c = bits(ctx.cycle.costs())
        a = ctx.answer(0)
        assert c[lo] == c[hi] and starts_now(a) and a[2] == [lo], (lo, hi, a)
        return dict(N=N, pair=(lo, hi), lanes=(lo % shape.block, hi % shape.block), cost_bits=c[lo], picked=a[2][0])
    return make(f"pair_{what}_n{N}_s{lo}_s{hi}", s_cluster(N, [lo, hi]), NO_NODE_FITS, S_PROBES, condition, [lo, hi], {"block"})


def s_walk(shape, N, c, nxt):
    """The walk's first candidate, node c (64 GiB), passes the front filter and its dip and fails the exact test: a reservation of
    4 GiB at [now + 100, now + 200) is the first entry below its front (the dip: 60 GiB, fits), one of 50 GiB at [now + 300, now + 400)
    leaves 14 GiB inside the probe's window of 1000 s.  nxt: the other 64 GiB node — or None: c is the last slot and the walk ends.
    Every reservation holds one raw cpu unit (the engine takes none without cpus), and nxt carries the same two with 4 GiB each: the
    same cost, bit for bit, and nothing in the way of a probe of half a cpu.
    CONDITION: the costs of c and nxt are the same bit pattern and c comes first in (cost, slot) order, or is the only candidate;
    the oracle's final map of c has 14 GiB at now + 300; the long probe starts now on nxt — or, without one, later on c itself, when
    the second reservation ends; a probe whose window ends at now + 300 starts now on c."""
    on = [c] + ([nxt] if nxt is not None else [])
    st, en, node, mem = [], [], [], []
    for n in on:
        st += [NOW + 100, NOW + 300]
        en += [NOW + 200, NOW + 400]
        node += [n, n]
        mem += [4 * GIB, (50 if n == c else 4) * GIB]
    z = [0] * len(node)
    rv = abi.Reservations(st, en, list(range(len(node) + 1)), node, [1] * len(node), mem, z, z, z)
    half = dict(cpu_raw=128)
    probes = [dict(half, L=1000, mem_gib=20), dict(half, L=300, mem_gib=20), dict(half, L=301, mem_gib=20), dict(half, L=100, mem_gib=100)]

    def condition(ctx):
        cb = bits(ctx.cycle.costs())
        tl = ctx.cycle.timeline(c)
        i = list(tl["t"]).index(NOW + 300)
        assert int(tl["mem"][i]) == 14 * GIB and int(tl["mem"][0]) == 64 * GIB and int(tl["mem"][1]) == 60 * GIB and int(tl["t"][1]) == NOW + 100, tl["mem"]
        a, short, edge = ctx.answer(0), ctx.answer(1), ctx.answer(2)
        assert starts_now(short) and short[2] == [c], short     # the entry at now + 300 is outside a window of 300 s
        if nxt is None:
            assert a[0] != 0 and a[1] == NOW + 400 and a[2] == [c] and edge[:3] == a[:3], (a, edge)
        else:
            assert cb[c] == cb[nxt] and c < nxt, (c, nxt)       # c is delivered first
            assert starts_now(a) and a[2] == [nxt] and starts_now(edge) and edge[2] == [nxt], (a, edge)
        return dict(N=N, first=c, next=nxt, long=a[:3], edge=edge[:3], cost_bits=cb[c])
    return make(f"walk_n{N}_c{c}_" + (f"x{nxt}" if nxt is not None else "end"), s_cluster(N, on), NO_NODE_FITS, probes, condition, on, {"block"},
                reservations=rv)


def family_s(shape):
    b = shape.block
    out = []
    for N in (b - 1, b, b + 1, 2 * b - 1, 2 * b, 2 * b + 1):
        for s in sorted({0, b - 1, b, N - 1}):
            if s < N:
                out.append(s_only(shape, N, s))
    N = 2 * b + 1
    for s in (0, b - 1, b):
        out.append(s_pair(shape, N, s, s + b, "lane"))
    out.append(s_pair(shape, N, 6, b + 6, "lane"))
    out.append(s_pair(shape, N, 6 + 1, b + 6, "wave"))   # (slots 7 and 70: 70 sits in lane 6, the lower lane holds the higher slot)
    out += [s_walk(shape, N, b - 1, b), s_walk(shape, N, 0, N - 1), s_walk(shape, N, N - 1, None)]
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# family K: node_num
# ---------------------------------------------------------------------------------------------------------------------------------
def k_sizes(n_p, k):
    """One core on the first min(k, n_p) nodes — all but the last where k >= n_p —, two on the others: a probe of up to two tasks a
    node collects one task from each of the first k candidates and two from every later one, which evicts a one-task node."""
    if k >= n_p:
        return [1] * (n_p - 1) + [2]
    return [1] * k + [2] * (n_p - k)


def k_nt(n_p, k):
    """ntasks at which the early break (hsize == k and hsum >= ntasks) holds exactly when the last counted candidate is pushed."""
    if k >= n_p:
        return n_p + 1 if k == n_p else k + 1        # all n_p candidates: n_p - 1 one-task nodes and the two-task one
    return k + min(2, n_p - k)                        # behind the first k: min(2, n_p - k) evictions


def k_idle(shape, n_p, k):
    """Probes of node_num k on an idle partition of n_p nodes (k_sizes): plain | ntasks = k_nt (the break exactly there) | one more
    (the break does not happen there) | exclusive | plain with more memory than any node has | one node.
    CONDITION (k <= n_p): the plain and the exclusive probe start now on the k lowest nodes; the exact twin starts now with k_nt tasks
    on a set that holds every two-core node counted; k > n_p: every probe is answered "Resource" without a start."""
    cores = k_sizes(n_p, k)
    nt = k_nt(n_p, k)
    tw = dict(cpu=1, L=100, k=k, tmin=1, tmax=2)
    probes = [dict(cpu=1, L=100, k=k), dict(tw, ntasks=nt), dict(tw, ntasks=nt + 1), dict(cpu=1, L=100, k=k, excl=1), dict(cpu=1, L=100, k=k, mem_gib=100),
              dict(cpu=1, L=50)]

    def condition(ctx):
        a = [ctx.answer(i) for i in range(5)]
        assert a[4][:3] == (abi.REASON_RESOURCE, 0, []) and starts_now(ctx.answer(5)), a[4]
        if k > n_p:
            assert all(x[:3] == (abi.REASON_RESOURCE, 0, []) for x in a), a
            return dict(n_p=n_p, k=k, answer="Resource")
        assert starts_now(a[0]) and a[0][2] == list(range(k)) and starts_now(a[3]) and a[3][2] == list(range(k)), (a[0][:2], a[3][:2])
        assert starts_now(a[1]) and sum(a[1][3]) == nt and len(a[1][2]) == k, a[1]
        twos = [n for n, t in zip(a[1][2], a[1][3]) if t == 2]
        want = list(range(k, nt)) if k < n_p else [n_p - 1]
        assert twos == want, (twos, want)
        return dict(n_p=n_p, k=k, ntasks=nt, evicted=len(twos) if k < n_p else 0, two_task_nodes=twos, plus_one=a[2][:2], plus_one_tasks=sum(a[2][3]))
    return make(f"k{k}_n{n_p}_idle", kat.cluster(cores, [16] * n_p), NO_NODE_FITS, probes, condition, [0, n_p - 1, min(k, n_p) - 1], {"block", "heap_ent_bytes"})


def k_busy(shape, n_p, k):
    """The same partition with n_p - k + 1 nodes (the highest ones) holding all but one raw cpu unit until now + 100 + 10 * i: k - 1 nodes
    are free now, the k-th comes free at a known key.
    CONDITION (k <= n_p): the plain, the two-task and the exclusive probe are backfilled (a reason, a start behind now) — the plain
    one to the earliest end among the busy nodes, now + 100; the one-node probe starts now."""
    cores = k_sizes(n_p, k)
    kk = min(k, n_p)
    busy = list(range(kk - 1, n_p))
    run = ss.running_of([(n, cores[n] * 256 - 1, NOW + 100 + 10 * i) for i, n in enumerate(busy)])
    probes = [dict(cpu=1, L=100, k=k), dict(cpu=1, L=100, k=k, ntasks=k + 1, tmin=1, tmax=2), dict(cpu=1, L=100, k=k, excl=1), dict(cpu=1, L=50)]

    def condition(ctx):
        a = [ctx.answer(i) for i in range(4)]
        if k > n_p:
            assert all(x[:3] == (abi.REASON_RESOURCE, 0, []) for x in a[:3]), a
            return dict(n_p=n_p, k=k, answer="Resource")
        assert a[0][0] != 0 and a[0][1] == NOW + 100 and len(a[0][2]) == k, a[0]
        assert a[2][0] != 0 and a[2][1] > NOW and len(a[2][2]) == k, a[2][:2]
        assert a[1][0] != 0 and (a[1][1] > NOW or a[1][:3] == (abi.REASON_RESOURCE, 0, [])), a[1][:2]
        assert (kk == 1) or starts_now(a[3]), a[3]
        return dict(n_p=n_p, k=k, plain=a[0][:2], two_task=a[1][:2], exclusive=a[2][:2])
    return make(f"k{k}_n{n_p}_busy", kat.cluster(cores, [16] * n_p), NO_NODE_FITS, probes, condition, busy[:3], {"block", "heap_ent_bytes"}, running=run)


def k_mixed(shape, n_p=None):
    """One probe of node_num n_p, 200 one-node probes around it, one of node_num n_p + 1 — on an idle partition of n_p = 2 * block + 1
    two-core nodes.  The expected answers are the same probes asked one at a time (probe_case.expected).  `plan`: the table again with
    CNS_PROBE_SCRATCH_CAP at two strides and at half a stride: grid 2 and grid 1, the answers unchanged.
    CONDITION: the wide probe starts now on every node; the one-node probes start now on node 0 or, asking for 100 GiB, nowhere; the
    too-wide probe is answered "Resource"; the stride is n_p + 1 entries."""
    n_p = n_p or 2 * shape.block + 1
    ones = [dict(cpu=1 + (i % 2), L=50 + i, mem_gib=100 if i % 50 == 49 else 1 + i % 7) for i in range(200)]
    probes = ones[:77] + [dict(cpu=1, L=100, k=n_p)] + ones[77:] + [dict(cpu=1, L=100, k=n_p + 1)]
    stride = n_p + 1
    per = stride * shape.heap_ent_bytes

    def condition(ctx):
        wide, too = ctx.answer(77), ctx.answer(len(probes) - 1)
        assert starts_now(wide) and wide[2] == list(range(n_p)) and too[:3] == (abi.REASON_RESOURCE, 0, []), (wide[:2], too)
        nowhere = 0
        for i in list(range(77)) + list(range(78, len(probes) - 1)):
            a = ctx.answer(i)
            if probes[i]["mem_gib"] == 100:
                assert a[:3] == (abi.REASON_RESOURCE, 0, []), (i, a)
                nowhere += 1
            else:
                assert starts_now(a) and a[2] == [0], (i, a)
        return dict(n_p=n_p, probes=len(probes), nowhere=nowhere, stride=stride, bytes_per_workgroup=per)
    return make(f"mixed_n{n_p}", idle(n_p, 2), NO_NODE_FITS, probes, condition, [0, n_p - 1], {"block", "heap_ent_bytes", "scratch_cap"},
                plan=[(None, None, stride), (2 * per, 2, stride), (per // 2, 1, stride)])


def family_k(shape):
    b = shape.block
    n = 2 * b + 1
    pairs = [(n, k) for k in (b - 1, b, b + 1, 2 * b, 2 * b + 1)] + [(np_, k) for np_ in (3, b + 1) for k in (np_ - 1, np_, np_ + 1)]
    out = []
    for n_p, k in pairs:
        out += [k_idle(shape, n_p, k), k_busy(shape, n_p, k)]
    return out + [k_mixed(shape)]


# ---------------------------------------------------------------------------------------------------------------------------------
# family T: node types
# ---------------------------------------------------------------------------------------------------------------------------------
def t_case(shape, busy):
    """max_types nodes with max_types distinct res_total records: node 0 has 8 cores, the last one 4, every node between them 2 and a
    memory of its own.  Probes of 3 cpus a task fit the first and the last node only: two tasks on node 0, one on the last.
    `busy`: both hold all but one raw cpu unit until now + 100 — the answers come from the res_total walk (ntasks_on_node_total).
    CONDITION: the oracle places the two-node probes on nodes 0 and T - 1 with 2 and 1 tasks, now or (busy) at now + 100; the one-node
    probe of two tasks goes to node 0; res_total differs between every two nodes."""
    T = shape.max_types
    cores = [8] + [2] * (T - 2) + [4]
    mem = [16 + i for i in range(T)]
    run = ss.running_of([(0, 8 * 256 - 1, NOW + 100), (T - 1, 4 * 256 - 1, NOW + 100)]) if busy else None
    probes = [dict(cpu=3, L=100, k=2, ntasks=3, tmin=1, tmax=2), dict(cpu=3, L=100, k=2, excl=1), dict(cpu=3, L=100, k=2, ntasks=3, tmin=1, tmax=2, excl=1),
              dict(cpu=3, L=100, k=1, ntasks=2, tmin=1, tmax=2), dict(cpu=3, L=100, k=3), dict(cpu=2, L=50)]
    want = NOW + 100 if busy else NOW

    def condition(ctx):
        assert len({(c, m) for c, m in zip(cores, mem)}) == T
        a = [ctx.answer(i) for i in range(len(probes))]
        for i in (0, 2):
            assert a[i][1] == want and (a[i][0] == 0) == (not busy) and a[i][2] == [0, T - 1] and a[i][3] == [2, 1], (i, a[i])
        assert a[1][1] == want and a[1][2] == [0, T - 1], a[1]
        assert a[3][1] == want and a[3][2] == [0] and a[3][3] == [2], a[3]
        assert a[4][:3] == (abi.REASON_RESOURCE, 0, []) and starts_now(a[5]), (a[4], a[5])
        return dict(types=T, busy=busy, tasks=a[0][3], exclusive_tasks=a[1][3], start=want - NOW)
    return make("types_busy" if busy else "types_idle", kat.cluster(cores, mem), NO_NODE_FITS, probes, condition, [0, T - 1], {"max_types"}, running=run)


def family_t(shape):
    return [t_case(shape, False), t_case(shape, True)]


# ---------------------------------------------------------------------------------------------------------------------------------
# family D: dips
# ---------------------------------------------------------------------------------------------------------------------------------
D_T = 500          # the dipped entry lies at now + D_T
D_G = 100          # ... and lasts this long
D_LAYOUT = dict(class_name=[0, 0, 1], class_shift=[0, 24, 48], class_width=[24, 24, 8])   # name 0: classes 0 and 1 (24 slots each); name 1: class 2


D_HOLD = dict(cpu_raw=1100)     # of node 0 until now + D_T where the case does not test cpus: the front has 948 units, the entry 1024


def d_case(shape, name, entry, refused, twins, covers, hold=None, mem0=64, by="queue"):
    """Node 0 (8 cores, mem0 GiB, 24 + 24 + 8 GRES slots) and a decoy (node 1: 3 cores — no queue job fits its total —, the same
    memory and GRES, all but one raw cpu unit held until now + 10, so it costs less than node 0 and hosts a probe ten seconds from now).
    `hold`: what a running allocation keeps of node 0 until now + D_T.  Queue job 0 asks for everything but `entry` (cpu_raw, mem
    bytes, [slots per class]) — more than the front has — and is backfilled to now + D_T for D_G seconds: the final map's entry there
    holds exactly `entry`.  Queue job 1 (`refused`: more than 3 cpus, and more than the entry has of whatever the case tests) fits the
    front, is refused now on node 0 by that one entry and backfilled: the refusal on which k_select posts the dip.
    by == "resv": a reservation [now + D_T, now + D_T + D_G) holds what queue job 0 would; the queue is the refused job alone.
    twins: [(probe spec, fits)] — fits: the oracle starts it now on node 0; else: it does not.
    CONDITION: queue job 1 is refused now and started later on node 0; the entry holds exactly `entry`; the twins start now on node 0 or do not."""
    ecpu, emem, egres = entry
    lay = abi.GresLayout(**D_LAYOUT)
    full = [24, 24, 8]
    slots = lambda cnt: sum(((1 << c) - 1) << s for c, s in zip(cnt, D_LAYOUT["class_shift"]))
    T_cpu, T_mem = 8 * 256, mem0 * GIB
    cluster = kat.cluster([8, 3], [mem0, mem0], gres=[slots(full), slots(full)], layout=lay)
    hold = hold or D_HOLD
    hg = hold.get("gres", [0, 0, 0])
    z = np.zeros(2, np.uint64)
    run = abi.Running(np.asarray([NOW + D_T, NOW + 10], np.int64), np.arange(3, dtype=np.uint32), np.asarray([0, 1], np.uint32),
                      np.asarray([hold.get("cpu_raw", 0), 3 * 256 - 1], np.int64), np.asarray([hold.get("mem", 0), 0], np.uint64), z, z.copy(),
                      np.asarray([slots(hg), 0], np.uint64))
    q0 = dict(cpu_raw=T_cpu - ecpu, mem=T_mem - emem, gspec=[f - e for f, e in zip(full, egres)], gtot=[48 - egres[0] - egres[1], 8 - egres[2]], L=D_G)
    q1 = dict(refused, L=D_T + 50)
    assert q1["cpu_raw"] > 3 * 256
    rv = None
    if by == "resv":
        rv = abi.Reservations([NOW + D_T], [NOW + D_T + D_G], [0, 1], [0], [q0["cpu_raw"]], [q0["mem"]], [0], [0], [slots(q0["gspec"])])
    queue = [q0, q1] if by == "queue" else [q1]
    qi = len(queue) - 1
    L0 = D_T + 1
    probes = []
    for spec, _ in twins:
        p = dict(spec)
        p.setdefault("L", L0)
        probes.append(p)

    def condition(ctx):
        pl = ctx.cycle.placements
        j1 = int(pl.start_sec[qi])
        if by == "queue":
            assert int(pl.start_sec[0]) == NOW + D_T and pl.reason[0] != 0 and int(pl.node_idx[0]) == 0, (name, pl.start_sec[0], pl.reason[0])
        assert pl.reason[qi] != 0 and j1 > NOW and int(pl.node_idx[qi]) == 0, (name, j1)
        tl = ctx.cycle.timeline(0)
        i = list(tl["t"]).index(NOW + D_T)
        g = int(tl["gres"][i])
        cnt = [bin((g >> s) & ((1 << w) - 1)).count("1") for s, w in zip(D_LAYOUT["class_shift"], D_LAYOUT["class_width"])]
        assert (int(tl["cpu_raw"][i]), int(tl["mem"][i]), cnt) == (ecpu, emem, list(egres)), (name, tl["cpu_raw"][i], tl["mem"][i], cnt)
        below = [k for k in range(1, i) if tl["cpu_raw"][k] < tl["cpu_raw"][0] or tl["mem"][k] < tl["mem"][0]]
        assert not below, (name, "an earlier entry below the front would take the dip", below)
        c = ctx.cycle.costs()
        assert c[1] < c[0], c
        for q, (spec, fits) in enumerate(twins):
            a = ctx.answer(q)
            assert (starts_now(a) and a[2] == [0]) == fits, (name, q, spec, fits, a)
        return dict(entry=(ecpu, emem, cnt), queue_job_1_start=j1 - NOW, answers=[ctx.answer(q)[:3] for q in range(len(twins))])
    return make(("dip_" if by == "queue" else "rdip_") + name, cluster, queue, probes, condition, [0, 1], covers, running=run, reservations=rv, dip=(0, D_T, by))


# A request for a class the layout does not define.  The reference looks at the layout's classes only (the oracle starts such a probe);
# the engine refuses the table, as cns_upload_jobs refuses such a queue: tests/test_gpu_probe_seams.py asserts the status and the text.
UNDEFINED_CLASS = dict(cpu=1, L=D_T + 1, gspec=[0, 0, 0, 1], gtot=[1])


def family_d(shape):
    return d_cases(shape, "queue") + d_cases(shape, "resv")


def d_cases(shape, by):
    d_case_ = d_case
    mk = lambda *a, **k: d_case_(*a, by=by, **k)
    c = 2
    sat = shape.dip_gres_sat
    msat = (shape.dip_mem_sat + 1) * GIB          # the first amount of memory whose GiB, rounded down, are above the saturated field
    cpu_frame = dict(entry=(c * 256 + 1, 63 * GIB, [24, 24, 8]), refused=dict(cpu_raw=1024), hold=dict(cpu_raw=600))
    rest = 63 * GIB
    out = [
        # the window's edge: an entry D_T seconds out is outside a window of D_T seconds
        mk(shape, "window", twins=[(dict(cpu_raw=c * 256 + 2, L=D_T), True), (dict(cpu_raw=c * 256 + 2, L=D_T + 1), False),
                                       (dict(cpu_raw=1024, L=D_T), True), (dict(cpu_raw=1024, L=D_T + 1), False)], covers={"loff_clamp"}, **cpu_frame),
        # cpus: the dip's are rounded up, the request's down
        mk(shape, "cpu", twins=[(dict(cpu_raw=c * 256 + 2), False), (dict(cpu_raw=c * 256 + 1), True)], covers={"dip_cpu_sat"}, **cpu_frame),
        # a time limit at and above the clamp reaches the dip like any window past it
        mk(shape, "loff", twins=[(dict(cpu_raw=c * 256 + 2, L=shape.loff_clamp), False), (dict(cpu_raw=c * 256 + 1, L=shape.loff_clamp), True),
                                     (dict(cpu_raw=c * 256 + 2, L=shape.loff_clamp + 1), False), (dict(cpu_raw=c * 256 + 1, L=shape.loff_clamp + 7), True),
                                     (dict(cpu_raw=c * 256 + 2, L=shape.loff_clamp - 1), False)], covers={"loff_clamp"}, **cpu_frame),
        # ... and a whole number of cpus at the entry, asked for exactly: the rounded request equals the rounded dip and fits
        mk(shape, "cpu_whole", (3 * 256, 63 * GIB, [24, 24, 8]), dict(cpu_raw=1024), [(dict(cpu_raw=3 * 256 + 1), False), (dict(cpu_raw=3 * 256), True)],
           {"dip_cpu_sat"}, hold=dict(cpu_raw=900)),
        # memory: 3 GiB + 1 byte
        mk(shape, "mem", (1024, 3 * GIB + 1, [24, 24, 8]), dict(cpu_raw=800, mem=3 * GIB + 2),
               [(dict(cpu=1, mem=3 * GIB + 2), False), (dict(cpu=1, mem=3 * GIB + 1), True)], {"dip_mem_sat"}),
        # ... and exactly 3 GiB, asked for exactly
        mk(shape, "mem_whole", (1024, 3 * GIB, [24, 24, 8]), dict(cpu_raw=800, mem=3 * GIB + 1),
           [(dict(cpu=1, mem=3 * GIB + 1), False), (dict(cpu=1, mem=3 * GIB), True)], {"dip_mem_sat"}),
        # memory saturation: the entry has more than dip_mem_sat GiB
        mk(shape, "mem_sat", (1024, msat + 5, [24, 24, 8]), dict(cpu_raw=800, mem=msat + 6),
               [(dict(cpu=1, mem=msat + 6), False), (dict(cpu=1, mem=msat + 5), True), (dict(cpu=1, mem=msat), True), (dict(cpu=1, mem=msat - 1), True)], {"dip_mem_sat"},
               mem0=shape.dip_mem_sat + 4465),
    ]
    # one class's nibble: sat - 1, sat, sat + 1, sat + 2 slots free at the entry against requests of sat, sat + 1, sat + 2
    for free in (sat - 1, sat, sat + 1, sat + 2):
        tw = [(dict(cpu=1, gspec=[need], gtot=[need]), need <= free) for need in (sat + 2, sat + 1, sat, sat - 1, sat + 3)]
        out.append(mk(shape, f"gres_free{free}", (1024, rest, [free, 24, 8]), dict(cpu_raw=800, gspec=[free + 1], gtot=[free + 1]), tw,
                          {"dip_gres_sat", "gres_classes"}, hold=dict(D_HOLD, gres=[3, 0, 0])))
    # a name's total over two classes: 7 + 8 unsaturated | 15 + 1 with one class saturated; requests by name only
    # ... | (sat + 2) + 1: the saturated class holds more than its nibble says, the sum of the nibbles is below a total that fits
    for a, b in ((sat // 2, sat - sat // 2), (sat, 1), (sat + 2, 1)):
        tw = [(dict(cpu=1, gtot=[need]), need <= a + b) for need in (a + b + 1, a + b, a + b - 1)]
        out.append(mk(shape, f"name_{a}_{b}", (1024, rest, [a, b, 8]), dict(cpu_raw=800, gtot=[a + b + 1]), tw, {"dip_gres_sat", "gres_names"}))
        if by == "queue":    # (k_wide posts no dip for a refusal by a name's total alone: behind a queue job this pair is plain parity, the rdip_ pair carries the filter)
            out[-1] = out[-1]._replace(dip=(0, D_T, "queue, by name"))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# family U: state nobody's selection kernel wrote
# ---------------------------------------------------------------------------------------------------------------------------------
def u_two_cycles(shape):
    """Two partitions of two nodes each (8 cores | 3: family D's frame in both), two cycles on one handle.  The first has jobs in both
    partitions and leaves a dipped entry in partition 1; the second has jobs in partition 0 only.  The probes go into partition 1.
    CONDITION: in the oracle's run of the second queue node 2's map is the snapshot's (one entry at now + D_T where the running
    allocation ends, none below the front), the big probe starts now on node 2 — which the first cycle's dip, were it still there,
    would refuse — and the first queue's run does hold the entry below the front."""
    cluster = kat.cluster([8, 3, 8, 3], [64] * 4, parts=[[0, 1], [2, 3]])
    z = np.zeros(4, np.uint64)
    run = abi.Running(np.asarray([NOW + D_T, NOW + 10, NOW + D_T, NOW + 10], np.int64), np.arange(5, dtype=np.uint32), np.arange(4, dtype=np.uint32),
                      np.asarray([600, 3 * 256 - 1, 600, 3 * 256 - 1], np.int64), z, z.copy(), z.copy(), z.copy())
    first = [dict(part=p, cpu_raw=8 * 256 - 513, L=D_G) for p in (0, 1)] + [dict(part=p, cpu_raw=1024, L=D_T + 50) for p in (0, 1)]
    second = [dict(part=0, cpu_raw=8 * 256 - 513, L=D_G), dict(part=0, cpu_raw=1024, L=D_T + 50)]
    probes = [dict(part=1, cpu_raw=1024, L=D_T + 50), dict(part=1, cpu_raw=514, L=D_T + 1), dict(part=1, cpu_raw=8 * 256, L=10), dict(part=0, cpu_raw=1024, L=D_T + 50)]

    def condition(ctx):
        quiet = ctx.run(pjobs(second + [dict(part=1, cpu=100000, L=1)]))     # (the oracle builds a partition's nodes when a job names it)
        tl = quiet.timeline(2)
        assert [int(t) for t in tl["t"]] == [NOW, NOW + D_T, INF] and int(tl["cpu_raw"][0]) == 8 * 256 - 600 and int(tl["cpu_raw"][1]) == 8 * 256, tl
        a = [ctx.answer(i) for i in range(4)]
        assert starts_now(a[0]) and a[0][2] == [2] and starts_now(a[1]) and a[1][2] == [2], a[:2]
        assert a[2][0] != 0 and a[2][1] == NOW + D_T and a[2][2] == [2] and a[3][0] != 0 and a[3][1] > NOW, a[2:]
        old = ctx.run(pjobs(first))
        t1 = old.timeline(2)
        i = list(t1["t"]).index(NOW + D_T)
        assert int(t1["cpu_raw"][i]) == 513 < int(t1["cpu_raw"][0]), t1["cpu_raw"]
        return dict(first_cycle_entry=int(t1["cpu_raw"][i]), answers=[x[:3] for x in a])
    return make("two_cycles", cluster, second, probes, condition, [0, 2], {"dip_cpu_sat"}, running=run, before=first, dip=(2, D_T, "queue"))


def u_empty_queue(shape):
    """Probes behind a cycle over an EMPTY queue, on a snapshot with running jobs: only k_init_nodes wrote the state.
    CONDITION: the oracle starts the small probe now on the idle node and backfills the wide one to the running allocation's end."""
    cluster = kat.cluster([4, 4], [16, 16])
    run = ss.running_of([(0, 3 * 256, NOW + 70)])
    probes = [dict(cpu=2, L=100), dict(cpu=2, L=100, k=2), dict(cpu=4, L=10, k=2, excl=1), dict(cpu=8, L=10)]

    def condition(ctx):
        a = [ctx.answer(i) for i in range(4)]
        assert starts_now(a[0]) and a[0][2] == [1] and a[1][0] != 0 and a[1][1] == NOW + 70 and a[1][2] == [0, 1], a[:2]
        assert a[2][1] == NOW + 70 and a[3][:3] == (abi.REASON_RESOURCE, 0, []), a[2:]
        return dict(answers=[x[:3] for x in a])
    return make("empty_queue", cluster, pjobs([]), probes, condition, [0, 1], {"block"}, running=run)


def family_u(shape):
    return [u_two_cycles(shape), u_empty_queue(shape)]


# ---------------------------------------------------------------------------------------------------------------------------------
# family V: reservations
# ---------------------------------------------------------------------------------------------------------------------------------
V_L = 1000


def v_first_resv(shape, off):
    """One node of 8 cores, 7 of them held by a running job until now + 200; a reservation of 6 cores from now + V_L + off to
    now + V_L + 1000.  A 4-core probe of V_L seconds fits the node from now + 200, but its window would reach the reservation, which
    leaves 2 cores: it starts when the reservation ends, at now + V_L + 1000, for off = 0 and for off = -1 alike.  The reason is
    "Resource Reserved" iff the node's first reservation begins before now + V_L (JobScheduler.cpp:6799-6806): for off = -1, not for 0.
    CONDITION: the oracle gives that start in both cases, "Resource" for off = 0 and "Resource Reserved" for off = -1."""
    cluster = kat.cluster([8], [32])
    rs, re_ = NOW + V_L + off, NOW + V_L + 1000
    rv = abi.Reservations([rs], [re_], [0, 1], [0], [6 * 256], [8 * GIB], [0x3F], [0], [0])
    run = ss.running_of([(0, 7 * 256, NOW + 200)])
    probes = [dict(cpu=4, L=V_L), dict(cpu=1, L=V_L), dict(cpu=1, L=10)]

    def condition(ctx):
        a = [ctx.answer(i) for i in range(3)]
        want = abi.REASON_RESOURCE_RESERVED if off < 0 else abi.REASON_RESOURCE
        assert a[0][:3] == (want, re_, [0]), (off, a[0])
        assert starts_now(a[1]) and starts_now(a[2]), a[1:]
        return dict(off=off, reason=a[0][0], start=a[0][1] - NOW)
    return make(f"first_resv_{'at' if off == 0 else 'before'}_L", cluster, NO_NODE_FITS, probes, condition, [0], {"block"}, running=run, reservations=rv)


def v_active(shape, where):
    """Probes into a reservation's own scheduler with now at rs - 1, rs, re - 1, re (the reservation: 6 of node 0's 8 cores).
    CONDITION: "Reservation Not Found" at rs - 1 and at re; inside, the probe starts now on node 0 and a probe of 7 cpus finds no node."""
    cluster = kat.cluster([8, 8], [32, 32])
    rs = NOW + {"rs-1": 1, "rs": 0, "re-1": -499, "re": -500}[where]
    re_ = rs + 500
    rv = abi.Reservations([rs], [re_], [0, 1], [0], [6 * 256], [8 * GIB], [0x3F], [0], [0])
    probes = [dict(cpu=2, L=1, resv=0), dict(cpu=7, L=1, resv=0), dict(cpu=2, L=100), dict(cpu=8, L=100, k=2)]
    inside = where in ("rs", "re-1")

    def condition(ctx):
        a = [ctx.answer(i) for i in range(4)]
        assert (rs <= NOW < re_) == inside
        if inside:
            assert starts_now(a[0]) and a[0][2] == [0] and a[1][:3] == (abi.REASON_RESOURCE, 0, []), a[:2]
        else:
            assert a[0][:3] == (abi.REASON_RESERVATION_NOT_FOUND, 0, []) and a[1][:3] == a[0][:3], a[:2]
        assert starts_now(a[2]), a[2]
        return dict(where=where, rs=rs - NOW, re=re_ - NOW, answers=[x[:3] for x in a])
    return make("active_" + {"rs-1": "before_rs", "rs": "at_rs", "re-1": "before_re", "re": "at_re"}[where], cluster, NO_NODE_FITS, probes, condition, [0, 1], {"block"}, reservations=rv)


def family_v(shape):
    return [v_first_resv(shape, 0), v_first_resv(shape, -1)] + [v_active(shape, w) for w in ("rs-1", "rs", "re-1", "re")]


# ---------------------------------------------------------------------------------------------------------------------------------
FAMILIES = {"RA": family_ra, "RC": family_rc, "RD": family_rd, "RB": family_rb, "S": family_s, "K": family_k, "T": family_t, "D": family_d,
            "U": family_u, "V": family_v}
KEEP = {"RB": False}       # family R-B's clusters are large and each is used once: built when asked for and not kept


def cases(shape, family):
    key = (shape, family)
    if key not in _CACHE:
        lst = FAMILIES[family](shape)
        assert len({c.name for c in lst}) == len(lst), "case names repeat"
        _CACHE[key] = {c.name: c for c in lst}
    return _CACHE[key]


def case_names(shape, family):
    return list(cases(shape, family))


def replay_groups(shape, family):
    """{select case: the names of its replays} of a family R: the splits of one select case share its snapshot."""
    out = {}
    for n in case_names(shape, family):
        out.setdefault(n.split("__")[0], []).append(n)
    return out


_MEMOS = {}


def memo_of(case):
    """The CycleMemo of a case's snapshot: one for all replays of one select case (they share its cluster object).  None for the large
    clusters of family R-B, whose runs are not worth keeping."""
    from tests import probe_case as pc
    if case.cluster.num_nodes > 256:
        return None
    key = id(case.cluster)
    if key not in _MEMOS:
        _MEMOS[key] = (case.cluster, pc.CycleMemo(case.cluster, case.now, running=case.running, reservations=case.reservations, **case.cfg))
    return _MEMOS[key][1]


def case(shape, family, name):
    d = cases(shape, family)
    c = d[name]
    if isinstance(c, LazyCase):
        c = c.build()
        if KEEP.get(family, True):
            d[name] = c
    return c
