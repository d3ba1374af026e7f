"""Cases on the seams of the serial protocol (csrc/wide_kernel.inc: k_wide<1> in serial-only mode — k_mem, the home workgroup alone, and
k_giant, the home with helper workgroups), every size taken from cns_serial_shape (engine.serial_shape()).  No HIP in here and no random
numbers.  Expected values never come from this file: tests/test_serial_seams.py runs the oracle on every case and asserts its CONDITION —
a function of the oracle's answers that states what puts the case on its seam —, tests/test_gpu_serial_seams.py holds the engine to the
oracle on the same cases.  The conventions are those of tests/select_seams.py; a case carries in addition `busy` (the partitions of its
launch that have jobs), `whole` (every partition has a job: the oracle builds every node) and `chain` (family Q: the cases run one after
the other on one handle).  `kernel` is (CNS_SELECT_KERNEL word or None, (what last_kernel() starts with, the helper count it names or None)).

Two facts put every seam within reach at small shapes: CNS_SELECT_KERNEL=giant routes every partition without preemption to k_giant (the
19-word instantiation), and with 17 or more busy partitions the same word yields k_mem (the 5-word one: fewer than helpers_min helpers).

The NEEDLE cluster: a partition of n one-core nodes, each held entirely until far in the future (6 days) by one running allocation, except
  free    slots that are free now (cost 0; {slot: cores} where a needle has more than one core),
  later   {slot: seconds}: held until now + seconds — they cost less than the far ones: what Phase B finds behind the needles,
  costly  {slot: seconds}: two cores, 255 raw units of them (no core ids) lent until now + seconds: free now for a one-cpu job, not
          wholly free, and a cost of seconds * 255 / 512 — needles that are NOT taken in slot order.
Slot s of partition 0 is node s.  pad(case, m) adds m one-node partitions with one one-cpu job each behind everything.

Families (L = scan_lanes, T = scan_trip_rows, HL = helper_lanes, HT = helper_trip_slots):
R  every case of families A, C, D of select_seams under `giant` (one partition: min(helpers_max, helper_budget) helpers) and as pad(case, 16) (k_mem)
N  node counts of one scan (L, T L, 64 L, each -1, +0, +1) with 16 busy partitions (k_giant, helpers_min helpers) and with 17 (k_mem)
H  helper stripes (k_giant)          W  the walk and the lists at 64 L + 1 nodes          G  shared groups (ALL + two subsets)
P  five partitions, two of them busy          Q  chains on one handle."""
from __future__ import annotations

import dataclasses
from collections import namedtuple

import numpy as np

from cranesched_amd import abi
from tests import kat
from tests import select_seams as ss

NOW = kat.NOW
GIB = 1 << 30
FAR = 6 * 86400     # the needle cluster's busy nodes are held this long (inside the seven-day window)
placed = ss.placed

Case = namedtuple("Case", "name cluster jobs now running cfg condition specs nodes covers kernel busy whole chain")
_CACHE = {}


def jobs_of(specs):
    """kat.jobs plus the node lists: `only` (include list) / `avoid` (exclude list) of a spec are lists of node indices."""
    j = kat.jobs(specs)
    if not any("only" in s or "avoid" in s for s in specs):
        return j
    kw = {}
    for key, field in (("only", "incl"), ("avoid", "excl")):
        off, flat = [0], []
        for s in specs:
            flat += list(s.get(key, ()))
            off.append(len(flat))
        kw[field + "_offsets"] = np.asarray(off, np.uint64)
        kw[field + "_nodes"] = np.asarray(flat or [0], np.uint32)
    return dataclasses.replace(j, **kw)


def make(name, cluster, specs, running, condition, nodes, covers, kernel, busy, whole=True, cfg=None, chain=None):
    return Case(name, cluster, jobs_of(specs), NOW, running, cfg or {}, condition, specs, tuple(int(n) for n in nodes), frozenset(covers), kernel, busy, whole, chain)


def plan_rule(shape, busy):
    """What `giant` launches for `busy` partitions: ("k_giant", helpers) or ("k_mem", None) — csrc/plan_host.inc, plan_serial_launch;
    tests/test_serial_seams.py holds this to the plan's own code."""
    nh = min(shape.helpers_max, shape.helper_budget // max(busy, 1))
    return ("k_giant", nh) if nh >= shape.helpers_min else ("k_mem", None)


def where(shape, rb, slot, nh=None):
    """The place of a slot in the loops of the job whose range starts at rb: the scanner's (row, lane, mask word, trip) and, with nh
    helpers, its helper, that helper's pass over the range and the trip of giant_scan the pass belongs to."""
    off = slot - rb
    row, lane = divmod(off, shape.scan_lanes)
    d = dict(row=row, lane=lane, word=row // 64, trip=row // shape.scan_trip_rows)
    if nh:
        stride = nh * shape.helper_lanes
        d.update(helper=(off % stride) // shape.helper_lanes, hpass=off // stride, htrip=off // stride // shape.helper_trip_slots)
    return d


# ---------------------------------------------------------------------------------------------------------------------------------
# the needle cluster
# ---------------------------------------------------------------------------------------------------------------------------------
def world(segments, parts=None):
    """segments: [(n, free, later, costly)] laid out one behind the other; parts: lists of node indices (None: one partition per
    segment).  Returns (cluster, running)."""
    cores, a_node, a_cpu, a_lo, a_end = [], [], [], [], []
    base, seg_nodes = 0, []
    for n, free, later, costly in segments:
        c = np.ones(n, np.int64)
        end = np.full(n, NOW + FAR, np.int64)
        cpu = np.full(n, 256, np.int64)
        lo = np.ones(n, np.uint64)
        held = np.ones(n, bool)
        for s, k in dict(free).items():
            c[s] = k
            held[s] = False
        for s, sec in dict(later).items():
            end[s] = NOW + sec
        for s, sec in dict(costly).items():
            c[s], end[s], cpu[s], lo[s] = 2, NOW + sec, 255, 0
        idx = np.nonzero(held)[0]
        cores.append(c)
        a_node.append(idx + base); a_cpu.append(cpu[idx]); a_lo.append(lo[idx]); a_end.append(end[idx])
        seg_nodes.append(np.arange(base, base + n))
        base += n
    cores = np.concatenate(cores)
    N = len(cores)
    parts = [np.asarray(p, np.uint32) for p in (parts if parts is not None else seg_nodes)]
    z = np.zeros(N, np.uint64)
    cluster = abi.Cluster(cores * 256, np.full(N, 16 * GIB, np.uint64), ((np.uint64(1) << cores.astype(np.uint64)) - np.uint64(1)).astype(np.uint64), z, z.copy(),
                          np.cumsum([0] + [len(p) for p in parts]).astype(np.uint32), np.concatenate(parts).astype(np.uint32))
    node, cpu, lo, end = (np.concatenate(x) for x in (a_node, a_cpu, a_lo, a_end))
    R = len(node)
    if R == 0:
        return cluster, None
    zr = np.zeros(R, np.uint64)
    running = abi.Running(end, np.arange(R + 1, dtype=np.uint32), node.astype(np.uint32), cpu, (cpu > 0).astype(np.uint64) * np.uint64(GIB), lo, zr, zr.copy())
    return cluster, running


def pad(case, m):
    """The case with m more nodes (one core, free), each a partition of its own with one one-cpu job behind the case's queue: m more busy
    partitions, nothing else changes.  CONDITION: the case's own, on the oracle's run of the padded case; every pad job starts now on its node."""
    c = case.cluster
    N, P = c.num_nodes, c.num_partitions
    ext = lambda a, v, dt: None if a is None else np.concatenate([np.asarray(a, dt), np.full(m, v, dt)])
    cluster = abi.Cluster(ext(c.cpu_total_raw, 256, np.int64), ext(c.mem_total, 16 * GIB, np.uint64), ext(c.core_lo, 1, np.uint64), ext(c.core_hi, 0, np.uint64),
                          ext(c.gres_slots, 0, np.uint64), np.concatenate([c.part_offsets, int(c.part_offsets[-1]) + 1 + np.arange(m, dtype=np.uint32)]).astype(np.uint32),
                          np.concatenate([c.part_nodes, N + np.arange(m, dtype=np.uint32)]).astype(np.uint32), gres=c.gres, schedulable=ext(c.schedulable, 1, np.uint8),
                          core_w2=ext(c.core_w2, 0, np.uint64), core_w3=ext(c.core_w3, 0, np.uint64), unsupported=ext(c.unsupported, 0, np.uint8))
    n0 = len(case.specs)
    specs = list(case.specs) + [dict(cpu=1, L=100, part=P + i) for i in range(m)]

    def condition(ora, nh=None):
        sub = lambda n=None: ora(n0 if n is None else n)                    # (the case's own queue is a prefix of the padded one)
        seen = case.condition(sub) if nh is None else case.condition(sub, nh)
        pl = ora().placements
        pads = [placed(pl, specs, n0 + i) for i in range(m)]
        assert pads == [(0, NOW, [N + i]) for i in range(m)], (case.name, pads)
        return dict(seen, pads=m)
    kernel = (case.kernel[0], case.kernel[1]) if case.kernel else None
    return Case(f"{case.name}_pad{m}", cluster, jobs_of(specs), case.now, case.running, case.cfg, condition, specs, case.nodes + (N, N + m - 1), case.covers, kernel,
                case.busy + m, case.whole, None)


def with_kernel(shape, case, word="giant"):
    """The case under `word` with the kernel the plan rule gives for its busy partitions."""
    return case._replace(kernel=(word, plan_rule(shape, case.busy)))


def needle_case(shape, name, n, free=(), later=(), costly=(), specs=(), expect=(), claims=(), covers=(), rb=0):
    """One needle partition of n nodes and a queue.  expect[j]: ("now", nodes) — reason none, start now, exactly these nodes (sorted) |
    ("wait", nodes or None) — a backfill reason and a start after now (on these nodes) | ("none",) — no nodes | None — unstated.
    claims: [(slot, {field: value})] — fields of where() the slot's name stands for; the GPU-side helper count is added by the caller.
    CONDITION: the oracle's answers are the expected ones and every claim follows from the shape's arithmetic."""
    free = dict(free) if isinstance(free, dict) else {s: 1 for s in free}
    cluster, running = world([(n, free, dict(later), dict(costly))])
    specs = list(specs)
    seam = sorted(set(free) | set(dict(later)) | set(dict(costly)) | {0, n - 1})

    def condition(ora, nh=None):
        pl = ora().placements
        got = [placed(pl, specs, j) for j in range(len(specs))]
        for j, e in enumerate(expect):
            if e is None:
                continue
            r, s, nd = got[j]
            if e[0] == "now":
                assert (r, s, nd) == (0, NOW, sorted(e[1])), (name, j, got[j], e)
            elif e[0] == "wait":
                assert r != 0 and s > NOW and nd and (e[1] is None or nd == sorted(e[1])), (name, j, got[j], e)
            else:
                assert nd == [] and s == 0 and r != 0, (name, j, got[j], e)
        for slot, claim in claims:
            assert rb <= slot < rb + n, (name, slot)
            w = where(shape, rb, slot, nh)
            assert all(w[k] == v for k, v in claim.items() if k in w), (name, slot, w, claim)
        return dict(n=n, rows=-(-n // shape.scan_lanes), answers=[(r, s - NOW if s else 0, nd) for r, s, nd in got])
    return make(name, cluster, specs, running, condition, seam, covers, None, 1)


def one(L=100, **kw):
    return dict(cpu=1, L=L, **kw)


# ---------------------------------------------------------------------------------------------------------------------------------
# family N
# ---------------------------------------------------------------------------------------------------------------------------------
def n_needles(shape, n):
    """{name: (slot, claim)} of the needles a partition of n nodes has."""
    L, T = shape.scan_lanes, shape.scan_trip_rows
    rows = -(-n // L)
    cand = [("r0_l0", 0, dict(row=0, lane=0, trip=0, word=0)), ("r0_lmax", L - 1, dict(row=0, lane=L - 1)),
            ("lastrow_first", (rows - 1) * L, dict(row=rows - 1, lane=0)), ("last", n - 1, dict(row=rows - 1, lane=(n - 1) % L)),
            ("trip0_end", (T - 1) * L + L - 1, dict(row=T - 1, lane=L - 1, trip=0)), ("trip1_first", T * L, dict(row=T, lane=0, trip=1)),
            ("word0_end", 63 * L + L - 1, dict(row=63, lane=L - 1, word=0)), ("word1_first", 64 * L, dict(row=64, lane=0, word=1))]
    out, seen = {}, set()
    for nm, slot, claim in cand:
        if 0 <= slot < n and slot not in seen:
            seen.add(slot)
            out[nm] = (slot, claim)
    return out


def n_cases(shape):
    L, T = shape.scan_lanes, shape.scan_trip_rows
    out = []
    sizes = [(L - 1, "L-1"), (L, "L"), (L + 1, "L+1"), (T * L - 1, "TL-1"), (T * L, "TL"), (T * L + 1, "TL+1"), (64 * L - 1, "64L-1"), (64 * L, "64L"), (64 * L + 1, "64L+1")]
    for n, tag in sizes:
        base_cov = {"scan_lanes"} | ({"scan_trip_rows"} if n >= T * L - 1 else set())
        nd = n_needles(shape, n)
        slots = sorted(s for s, _ in nd.values())
        claims = list(nd.values())
        # one: the lower half of the needles costs nothing (taken in slot order), the upper half is `costly`, the highest slot the cheapest
        # (taken highest slot first); one more job finds every needle taken and is backfilled
        half = (len(slots) + 1) // 2
        plain, dear = slots[:half], slots[half:]
        costly = {s: 10 * (len(dear) - i) for i, s in enumerate(dear)}
        order = plain + dear[::-1]
        one_case = needle_case(shape, f"one_{tag}", n, free=plain, costly=costly, specs=[one() for _ in order] + [one()],
                               expect=[("now", [s]) for s in order] + [("wait", None)], claims=claims, covers=base_cov)
        # pair: two needles as far apart as the partition allows (another mask word, else another trip, else another lane) and a job of
        # two nodes: the second node comes from the masks; the one-node job behind it waits
        a, b = slots[1] if len(slots) > 2 else slots[0], slots[-1]
        pair_case = needle_case(shape, f"pair_{tag}", n, free=[a, b], specs=[one(k=2), one()], expect=[("now", [a, b]), ("wait", None)],
                                claims=[(a, where(shape, 0, a)), (b, where(shape, 0, b))], covers=base_cov)
        # phantom: slot 0 alone is free, the job wants two nodes: never [0, 0]
        ph_case = needle_case(shape, f"phantom_{tag}", n, free=[0], specs=[one(k=2), one()], expect=[None, None], claims=[(0, dict(row=0, lane=0))], covers=base_cov)
        ph_inner = ph_case.condition

        def ph_condition(ora, nh=None, inner=ph_inner, nm=f"phantom_{tag}", specs=ph_case.specs):
            seen = inner(ora, nh)
            r, s, nd = placed(ora().placements, specs, 0)
            assert (r != 0) and len(set(nd)) == len(nd) and (nd == [] or (len(nd) == 2 and s > NOW)), (nm, r, s, nd)   # refused, or backfilled onto two different nodes
            assert placed(ora().placements, specs, 1) == (0, NOW, [0]) or nd, nm
            return seen
        ph_case = ph_case._replace(condition=ph_condition)
        for c in (one_case, pair_case, ph_case):
            for m, inst in ((shape.helper_budget // shape.helpers_min - 1, "giant"), (shape.helper_budget // shape.helpers_min, "mem")):
                words = {"giant": {"giant_mem_words", "giant_mem_slots", "helpers_min", "helper_budget"}, "mem": {"mem_words", "mem_slots", "helpers_min"}}[inst]
                p = with_kernel(shape, pad(c, m))
                assert p.kernel[1][0] == ("k_giant" if inst == "giant" else "k_mem")
                out.append(bind_nh(p._replace(name=f"{c.name}_{inst}", covers=p.covers | (words if n >= 64 * L - 1 else {"helpers_min"}))))
    return out


def bind_nh(case):
    """The case with its condition bound to the helper count its kernel names (where()'s helper fields)."""
    nh = case.kernel[1][1]
    inner = case.condition

    def condition(ora):
        return inner(ora) if nh is None else inner(ora, nh)
    return case._replace(condition=condition)


# ---------------------------------------------------------------------------------------------------------------------------------
# family H
# ---------------------------------------------------------------------------------------------------------------------------------
def h_single(shape, name, n, slot, claim, pads, covers):
    c = needle_case(shape, name, n, free=[slot], specs=[one(), one()], expect=[("now", [slot]), ("wait", None)], claims=[(slot, claim)], covers=covers)
    if pads:
        c = pad(c, pads)._replace(name=name)
    c = with_kernel(shape, c)
    want = plan_rule(shape, 1 + pads)
    inner = c.condition

    def condition(ora):
        assert c.kernel[1] == want and want[0] == "k_giant", (name, want)
        return dict(inner(ora, want[1]), nh=want[1])
    return c._replace(condition=condition)


def h_cases(shape):
    HL, HT, L = shape.helper_lanes, shape.helper_trip_slots, shape.scan_lanes
    out = []
    cov = {"helper_lanes", "helper_trip_slots", "helpers_min", "helper_budget"}
    nh = shape.helpers_min
    pads = shape.helper_budget // nh - 1                    # 16 busy partitions
    assert plan_rule(shape, 1 + pads) == ("k_giant", nh) and plan_rule(shape, 2 + pads)[0] == "k_mem"
    for n, tag in ((HL * nh - 1, "pass-1"), (HL * nh + 1, "pass+1"), (HT * HL * nh - 1, "trip-1"), (HT * HL * nh + 1, "trip+1")):
        for h in range(nh):
            slot = min(h * HL + 7 + h, n - 1) if h < nh - 1 else n - 1 if n < HL * nh else h * HL + HL - 1   # (the last helper: its last lane, or the partition's last slot)
            out.append(h_single(shape, f"stripe_{tag}_h{h}", n, slot, dict(helper=h, hpass=0, htrip=0), pads, cov))
        if n > HL * nh:                                     # the first slot of every helper's second pass; at the trip sizes also the last slot: pass HT - 1 or the second trip
            out.append(h_single(shape, f"stripe_{tag}_pass1", n, HL * nh, dict(helper=0, hpass=1, htrip=0), pads, cov))
        if n > HT * HL * nh:
            out.append(h_single(shape, f"stripe_{tag}_trip1", n, HT * HL * nh, dict(helper=0, hpass=HT, htrip=1), pads, cov))
        elif n == HT * HL * nh - 1:
            out.append(h_single(shape, f"stripe_{tag}_last", n, n - 1, dict(helper=nh - 1, hpass=HT - 1, htrip=0), pads, cov))
        if n > HL * nh:
            # equal costs in two helpers' stripes: helper 1's first slot is below helper 0's second pass — the lower slot wins, twice
            a, b = HL, HL * nh
            c = needle_case(shape, f"tie_{tag}", n, free=[a, b], specs=[one(), one(), one()], expect=[("now", [a]), ("now", [b]), ("wait", None)],
                            claims=[(a, dict(helper=1, hpass=0)), (b, dict(helper=0, hpass=1))], covers=cov)
            out.append(bind_nh(with_kernel(shape, pad(c, pads)._replace(name=f"tie_{tag}"))))
            # ... and in ONE helper lane's own passes (the same lane meets both, the later one in its second pass or its second trip)
            b = HT * HL * nh if n > HT * HL * nh else HL * nh
            c = needle_case(shape, f"tie_lane_{tag}", n, free=[0, b], specs=[one(), one(), one()], expect=[("now", [0]), ("now", [b]), ("wait", None)],
                            claims=[(0, dict(helper=0, hpass=0, lane=0)), (b, dict(helper=0, hpass=b // (HL * nh), htrip=b // (HT * HL * nh)))], covers=cov)
            out.append(bind_nh(with_kernel(shape, pad(c, pads)._replace(name=f"tie_lane_{tag}"))))
    for busy in (3, 5, 7):                                  # helper counts that are no power of two: a needle in the last helper's stripe and one in its second pass
        k = plan_rule(shape, busy)[1]
        n = 2 * k * HL + 1
        slot = (k - 1) * HL + HL - 1
        out.append(h_single(shape, f"odd_nh{k}_last", n, slot, dict(helper=k - 1, hpass=0), busy - 1, cov))
        out.append(h_single(shape, f"odd_nh{k}_pass1", n, k * HL + slot, dict(helper=k - 1, hpass=1), busy - 1, cov))
    top = min(shape.helpers_max, shape.helper_budget)
    cov1 = {"helper_lanes", "helpers_max", "helper_budget"}
    small = HL - 212
    out.append(h_single(shape, "one_part_small", small, small - 1, dict(helper=0, hpass=0, row=0), 0, cov1))   # every helper but the first answers "none"
    for n, tag in ((HL * top - 1, "-1"), (HL * top + 1, "+1")):
        out.append(h_single(shape, f"one_part_full{tag}_last", n, n - 1, dict(helper=(n - 1) % (HL * top) // HL, hpass=(n - 1) // (HL * top)), 0, cov1))
        out.append(h_single(shape, f"one_part_full{tag}_h{top - 1}", n, (top - 1) * HL, dict(helper=top - 1, hpass=0), 0, cov1))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# family W
# ---------------------------------------------------------------------------------------------------------------------------------
def w_cases(shape):
    L = shape.scan_lanes
    n = 64 * L + 1
    w0, w1 = 63 * L + L - 1, 64 * L            # the last slot of mask word 0 | the one slot of word 1
    cov = {"scan_lanes", "scan_trip_rows"}
    inner = []
    # window: X (word 0) is free and costs nothing, Y is held for 50 s, Z (word 1) is a costly needle.  Job 0 wants two nodes and all their memory (Z lends a GiB): Phase A has X
    # alone, Phase B takes X and Y at now + 50.  Job 1 (100 s): round 0 is X — 100 by now, below Z's 149.4 —, free in front, busy inside
    # the window: the exact test refuses, the next candidate is Z, in the other word.  Job 2 (50 s) ends on the key: X, now.
    X, Y, Z = w0, 5, w1
    inner.append(needle_case(shape, "window", n, free=[X], later={Y: 50}, costly={Z: 300}, specs=[one(k=2, mem_gib=16), one(), one(L=50), one()],
                             expect=[("wait", [X, Y]), ("now", [Z]), ("now", [X]), ("wait", None)], claims=[(X, dict(word=0, row=63)), (Z, dict(word=1, row=64))], covers=cov))
    # ntasks > node_num: needles of 1, 1 and 3 cores, the last in word 1; four tasks on two nodes: the walk drops the first needle for the third
    A, B, C_ = 3, w0, w1
    inner.append(needle_case(shape, "ntasks", n, free={A: 1, B: 1, C_: 3}, specs=[dict(cpu=1, L=100, k=2, ntasks=4, tmin=1, tmax=3), one(), one(), one()],
                             expect=[("now", [B, C_]), None, None, None], claims=[(B, dict(word=0)), (C_, dict(word=1))], covers=cov))
    # exclusive: E1 (word 0) lends a unit — free for a one-cpu job, not wholly free —, E2 (word 1) is free: the first exclusive job takes E2,
    # the second is backfilled onto E1 behind the loan (now + 10); a plain job of 10 s still starts on E1 now, one of 11 s does not
    E1, E2 = L - 1, w1
    inner.append(needle_case(shape, "exclusive", n, costly={E1: 10}, free=[E2], specs=[one(excl=1), one(excl=1), one(L=10), one(L=11)],
                             expect=[("now", [E2]), ("wait", [E1]), ("now", [E1]), ("wait", None)], claims=[(E1, dict(row=0, lane=L - 1)), (E2, dict(word=1))], covers=cov))
    # Phase B: a three-node job; Phase A walks the two needles — X2 in word 1, the costly Z2 in word 0 — marks both and runs out; Phase B restarts
    # from the res_total minimum (X2) and must take Z2 AGAIN from the masks (the `used` marks of Phase A are gone), then the cheapest held node
    X2, Z2, Y2, Y3 = w1, L - 1, w0, 7
    inner.append(needle_case(shape, "phase_b", n, free=[X2], costly={Z2: 20}, later={Y2: 50, Y3: 60}, specs=[one(k=3), one(L=50), one()],
                             expect=[("wait", [X2, Z2, Y2]), ("now", [Z2]), None], claims=[(X2, dict(word=1)), (Z2, dict(word=0, row=0)), (Y2, dict(word=0, row=63))], covers=cov))
    # lists: needles in rows 63 and 64 (the word boundary of list_mask's rows); include- and exclude-list jobs one for one with plain jobs,
    # whose answers depend on what the listed jobs took
    r63 = [63 * L, 63 * L + 1, w0]
    inner.append(needle_case(shape, "lists", n, free=r63 + [w1], specs=[one(only=[w0, w1]), one(), one(avoid=[63 * L + 1]), one(), one(only=[w1]), one(avoid=[0, w0]), one()],
                             expect=[("now", [w0]), ("now", [63 * L]), ("now", [w1]), ("now", [63 * L + 1]), ("wait", [w1]), ("wait", None), ("wait", None)],
                             claims=[(63 * L, dict(row=63, lane=0, word=0)), (w0, dict(row=63, word=0)), (w1, dict(row=64, word=1))], covers=cov))
    out = []
    for c in inner:
        out.append(bind_nh(with_kernel(shape, c)._replace(name=c.name + "_giant", covers=c.covers | {"giant_mem_words", "helpers_max"})))
        p = with_kernel(shape, pad(c, shape.helper_budget // shape.helpers_min))
        out.append(bind_nh(p._replace(name=c.name + "_mem", covers=c.covers | {"mem_words", "helpers_min"})))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# family G
# ---------------------------------------------------------------------------------------------------------------------------------
def g_group(shape, name, n, a, b, free, specs, expect, claims, covers, kernel_word, pads=0):
    """ALL over n nodes, member A = nodes [0, a), member B = nodes [a, a + b): one group of n + a + b slots; ALL's slots come first, then A's,
    then B's (the job's own range starts at rb = 0, n, n + a).  claims: [(member, node, {field: value})]."""
    assert a + b <= n
    cluster, running = world([(n, {s: 1 for s in free}, {}, {})], parts=[np.arange(n), np.arange(a), np.arange(a, a + b)])
    rbs = (0, n, n + a)
    lo = (0, 0, a)

    def condition(ora):
        pl = ora().placements
        got = [placed(pl, specs, j) for j in range(len(specs))]
        for j, e in enumerate(expect):
            r, s, nd = got[j]
            if e[0] == "now":
                assert (r, s, nd) == (0, NOW, sorted(e[1])), (name, j, got[j], e)
            else:
                assert r != 0 and s != NOW, (name, j, got[j], e)
        assert n + a + b == int(cluster.part_offsets[-1])
        for member, node, claim in claims:
            slot = rbs[member] + node - lo[member]
            w = where(shape, rbs[member], slot)
            assert all(w[k] == v for k, v in claim.items()), (name, member, node, w, claim)
        L, HL = shape.scan_lanes, shape.helper_lanes
        return dict(slots=n + a + b, rb=rbs, rb_mod_lanes=[x % L for x in rbs], rb_mod_helper_lanes=[x % HL for x in rbs], answers=[(r, s - NOW if s else 0, nd) for r, s, nd in got])
    c = make(name, cluster, specs, running, condition, sorted(set(free) | {0, n - 1}), covers, None, 1)
    if pads:
        c = pad(c, pads)._replace(name=name)
    return c._replace(kernel=kernel_word)


def g_cases(shape):
    L, HL, tile = shape.scan_lanes, shape.helper_lanes, shape.select_tile_slots
    out = []
    # the routing seam under the default word: the group's slots at k_select's widest tile | one more
    for slots, kern in ((tile, ("k_select<", None)), (tile + 1, ("k_mem", None))):
        n = (slots + 1) // 2
        a = 4000
        b = slots - n - a
        assert 0 < b and a + b <= n
        free = [0, a - 1, a, a + b - 1]
        specs = [one(part=2), one(part=1), one(part=0), one(part=1), one(part=2), one(part=2), one(part=0)]
        expect = [("now", [a]), ("now", [0]), ("now", [a - 1]), ("wait",), ("now", [a + b - 1]), ("wait",), ("wait",)]
        out.append(g_group(shape, f"route_{slots}", n, a, b, free, specs, expect, [], {"select_tile_slots"}, (None, kern)))
    # rb off every multiple of the lanes: ALL = 1000 nodes, A = 333, B = 555; needles on the first and last slot of A's and of B's range and
    # one node that only ALL has.  B's jobs must not take A's free nodes (free in ALL's range and in A's), A's not B's; ALL's job takes the
    # lowest free node whoever else has it.
    n, a, b = 1000, 333, 555
    assert all(x % L and x % HL for x in (n, n + a))
    only_all = a + b + 10
    free = [0, a - 1, a, a + 7, a + b - 1, only_all]
    # (the two-node jobs take their second node from the masks: `used` marks the first by its row in the job's OWN range)
    specs = [one(part=2, k=2), one(part=1, k=2), one(part=2), one(part=2), one(part=0), one(part=1), one(part=0)]
    expect = [("now", [a, a + 7]), ("now", [0, a - 1]), ("now", [a + b - 1]), ("wait",), ("now", [only_all]), ("wait",), ("wait",)]
    claims = [(2, a, dict(row=0, lane=0)), (2, a + b - 1, dict(row=(b - 1) // L, lane=(b - 1) % L)), (1, 0, dict(row=0, lane=0)), (1, a - 1, dict(row=0, lane=a - 1))]
    cov = {"scan_lanes", "helper_lanes"}
    out.append(g_group(shape, "members_giant", n, a, b, free, specs, expect, claims, cov | {"helpers_max"}, ("giant", plan_rule(shape, 1))))
    pads = shape.helper_budget // shape.helpers_min
    out.append(g_group(shape, "members_mem", n, a, b, free, specs, expect, claims, cov | {"helpers_min"}, ("giant", plan_rule(shape, 1 + pads)), pads=pads))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# family P
# ---------------------------------------------------------------------------------------------------------------------------------
def p_case(shape):
    """Five partitions, jobs in partitions 1 and 3 only (widths L + 1 and helper_lanes * 2 + 3): the launch maps its two busy partitions
    through part_map, GiantCtl is indexed by the partition.  Partition 1's needles are taken lowest slot first, partition 3's — costly —
    highest slot first.  CONDITION: those orders; the two busy partitions get helper_budget / 2 helpers."""
    L, HL = shape.scan_lanes, shape.helper_lanes
    w = [9, L + 1, 3, 2 * HL + 3, 5]
    base = np.cumsum([0] + w)
    f1 = [0, L - 1, L]
    c3 = {1: 30, HL: 20, 2 * HL + 2: 10}
    segs = [(w[0], {0: 1}, {}, {}), (w[1], {s: 1 for s in f1}, {}, {}), (w[2], {1: 1}, {}, {}), (w[3], {}, {}, c3), (w[4], {4: 1}, {}, {})]
    cluster, running = world(segs)
    specs = [one(part=3), one(part=1), one(part=3), one(part=1), one(part=3), one(part=1), one(part=1), one(part=3)]
    n1 = [int(base[1]) + s for s in f1]
    n3 = [int(base[3]) + s for s in sorted(c3, reverse=True)]
    want = [n3[0], n1[0], n3[1], n1[1], n3[2], n1[2]]
    kern = plan_rule(shape, 2)

    def condition(ora):
        pl = ora().placements
        got = [placed(pl, specs, j) for j in range(len(specs))]
        assert got[:6] == [(0, NOW, [x]) for x in want], (got, want)
        assert all(r != 0 and s > NOW for r, s, _ in got[6:]), got[6:]
        assert kern == ("k_giant", shape.helper_budget // 2)
        return dict(widths=w, answers=[(r, s - NOW if s else 0, nd) for r, s, nd in got], nh=kern[1])
    return make("two_of_five", cluster, specs, running, condition, n1 + n3, {"scan_lanes", "helper_lanes", "helper_budget"}, ("giant", kern), 2, whole=False)


# ---------------------------------------------------------------------------------------------------------------------------------
# family Q
# ---------------------------------------------------------------------------------------------------------------------------------
def q_case(shape):
    """One handle under `giant`: a family-H case (16 busy partitions); a different, shorter queue on the same snapshot (its one job is a
    two-node job: another answer for the same needle's node, and one busy partition — 64 helpers where there were 4); a queue on another
    cluster with three busy partitions.  Every cycle is held to the oracle on its own: an answer, a helper tag or a sequence word left
    over from the cycle before shows.  CONDITION: each link's own; the helper counts differ from link to link."""
    hs = cases(shape, "H")
    first = hs["tie_pass+1"]
    n0 = len(first.specs) - (first.busy - 1)
    specs = [one(k=2, L=70)]
    needles = [shape.helper_lanes, shape.helper_lanes * shape.helpers_min]   # the two needles of tie_pass+1

    def cond2(ora):
        r, s, nd = placed(ora().placements, specs, 0)
        assert r == 0 and s == NOW and nd == needles, (r, s, nd)
        return dict(nodes=nd)
    second = Case("same_snapshot_shorter_queue", first.cluster, jobs_of(specs), NOW, first.running, {}, cond2, specs, first.nodes, first.covers,
                  ("giant", plan_rule(shape, 1)), 1, False, None)
    third = hs["odd_nh21_pass1"] if "odd_nh21_pass1" in hs else next(c for n, c in hs.items() if n.startswith("odd_nh"))
    chain = (first, second, third)

    def condition(ora_of):
        seen = [c.condition(ora_of(c)) for c in chain]
        nhs = [c.kernel[1][1] for c in chain]
        assert len(set(nhs)) == 3 and n0 == 3, (nhs, n0)
        return dict(links=[c.name for c in chain], nh=nhs, seen=seen)
    return Case("three_cycles", None, None, NOW, None, {}, condition, None, (), frozenset({"helpers_min", "helpers_max", "helper_budget"}), ("giant", None), 0, False, chain)


# ---------------------------------------------------------------------------------------------------------------------------------
# family R
# ---------------------------------------------------------------------------------------------------------------------------------
def r_case(shape, sel_case, padded):
    """A select-seam case as a serial case: unchanged under `giant` (one partition, the most helpers a launch gives), or pad(case, 16)."""
    c = Case(*sel_case[:10], None, 1, True, None)
    if padded:
        c = pad(c, shape.helper_budget // shape.helpers_min)
    return with_kernel(shape, c)._replace(covers=frozenset({"helpers_min", "helper_budget"} if padded else {"helpers_max", "helper_budget"}))


def r_cases(shape, sel_shape, fam, padded):
    return [r_case(shape, c, padded) for c in ss.cases(sel_shape, fam).values()]


# ---------------------------------------------------------------------------------------------------------------------------------
FAMILIES = {"N": n_cases, "H": h_cases, "W": w_cases, "G": g_cases, "P": lambda s: [p_case(s)], "Q": lambda s: [q_case(s)]}
REPLAYED = ("A", "C", "D")


def cases(shape, family):
    """The cases of a family for that shape, built once per process: {name: Case} in a fixed order.  Families RA, RC, RD (`_pad`: k_mem)
    replay select_seams' families for ss.SHIPPED."""
    key = (shape, family)
    if key not in _CACHE:
        if family[0] == "R":
            lst = r_cases(shape, ss.SHIPPED, family[1], family.endswith("_pad"))
        else:
            lst = FAMILIES[family](shape)
        assert len({c.name for c in lst}) == len(lst), "case names repeat"
        _CACHE[key] = {c.name: c for c in lst}
    return _CACHE[key]


def case_names(shape, family):
    return list(cases(shape, family))


def case(shape, family, name):
    return cases(shape, family)[name]


R_FAMILIES = tuple(f"R{f}{p}" for f in REPLAYED for p in ("", "_pad"))
# The shipped shape (tests/test_serial_abi.py pins it): the lists pytest parametrizes over are built for it at import, without the library.
SHIPPED = abi.SerialShape(448, 4, 5, 19, 143360, 544768, 512, 4, 64, 64, 4, 16576)
