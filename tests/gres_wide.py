"""Wide GRES layouts: scenarios at the engine's GRES limits (node_select.h: up to 64 slots in up to 8 (name, type) classes under up
to 4 names, up to 64 distinct res_total records per snapshot) and the checks that a case really reaches those edges.

The hot path keeps GRES counts in compressed forms with saturating rules (4-bit class counts that stop at 15, a request total capped
at 15, the predicted front after a selection that keeps a saturated count).  `tests.helpers.random_case` never has a class of more
than 8 slots, so none of those rules ever saturates there; the cases here hold classes of 16 to 64 slots, bit 63, names 2 and 3, and
requests around 15 / 16 / the class width / 64 / 127 / 128 / 255.

Calls held to their truth on these layouts: the selection kernels, reservations, preemption, the run limits, the step scheduler and
the group (tests/test_gpu_gres_wide.py); cns_probe (probe_case, probe_dip_kat), cns_validate_jobs (gres_wide_case's queue and the
hand tables of tests/valid_case.hand_wide), cns_check_submissions (submit_case, tests/submit_case.hand_table_wide), and the device
ledger — cns_running_seed / _advance, their _attrs forms and cns_running_select_preempt (tests/running_case.scenario through
wide_case_of, preempt_case) — in tests/test_gpu_gres_wide_calls.py.  Not covered on purpose: cns_usage_apply (its device code takes the
4 + 8 GRES components as plain numbers and its own tests fill all twelve), cns_commit_check, cns_gate_pending and cns_resvq_run (they
read no GRES)."""
from __future__ import annotations

import numpy as np

from cranesched_amd import abi, synth

GIB = 1 << 30
M64 = (1 << 64) - 1

# (class_name, class_shift, class_width) per class, in class-index order
LAYOUTS = {
    # one class of 64 slots: bit 63 is a slot
    "one64": ([0], [0], [64]),
    # 8 classes of 8 under names 0..3, two per name; class index and bit position disagree
    "eight_by_8_four_names": ([3, 0, 2, 1, 0, 3, 1, 2], [56, 8, 40, 0, 24, 48, 16, 32], [8] * 8),
    # uneven widths with gaps: name 0 has three classes (1, 5, 16 slots: dyn_gres, gmode 4), name 1 one class of 17, name 2 one
    # class of 21 that ends at bit 63
    "uneven": ([0, 1, 0, 0, 2], [0, 2, 20, 26, 43], [1, 17, 5, 16, 21]),
}
NAMED = sorted(LAYOUTS)


def make_layout(name: str | int) -> abi.GresLayout:
    """A named layout, or (an int) the random layout of that seed."""
    if isinstance(name, str):
        n, s, w = LAYOUTS[name]
        return abi.GresLayout(class_name=list(n), class_shift=list(s), class_width=list(w))
    return random_layout(name)


def random_layout(seed: int) -> abi.GresLayout:
    """1..8 classes under 1..4 names, widths 1..64, no overlaps, at most 64 bits in all; class order shuffled against bit order."""
    rng = np.random.default_rng(77_000 + seed)
    C = int(rng.integers(1, 9))
    while True:
        w = rng.integers(1, 65, C)
        if w.sum() <= 64:
            break
        w = np.maximum(1, (w * (64 / w.sum()) * rng.uniform(0.5, 1.0))).astype(np.int64)
        if w.sum() <= 64:
            break
    gaps = rng.multinomial(64 - int(w.sum()), np.ones(C + 1) / (C + 1))
    shifts, pos = [], 0
    for c in range(C):
        pos += int(gaps[c])
        shifts.append(pos)
        pos += int(w[c])
    names = rng.integers(0, int(rng.integers(1, 5)), C)
    perm = rng.permutation(C)
    return abi.GresLayout(class_name=[int(names[p]) for p in perm], class_shift=[shifts[p] for p in perm],
                          class_width=[int(w[p]) for p in perm])


def class_masks(lay: abi.GresLayout) -> list[int]:
    return [(((1 << w) - 1) << s) & M64 for s, w in zip(lay.class_shift, lay.class_width)]


def class_counts(lay: abi.GresLayout, g: int) -> list[int]:
    return [bin(g & m).count("1") for m in class_masks(lay)]


def _gres_kinds(lay: abi.GresLayout, rng, K: int) -> list[int]:
    """K distinct node slot masks: all slots, nothing, whole classes, the low part of classes, random subsets."""
    cm = class_masks(lay)
    full = 0
    for m in cm:
        full |= m
    kinds = [full, 0]
    tries = 0
    while len(kinds) < K and tries < 10_000:
        tries += 1
        g = 0
        style = int(rng.integers(0, 3))
        for s, w, m in zip(lay.class_shift, lay.class_width, cm):
            r = rng.random()
            if style == 0:                                     # whole classes or nothing
                g |= m if r < 0.6 else 0
            elif style == 1:                                   # the lowest n slots of a class
                n = int(rng.integers(0, w + 1))
                g |= ((1 << n) - 1) << s
            else:                                              # a random subset, dense
                keep = int(rng.integers(0, 1 << 62)) | (int(rng.integers(0, 4)) << 62)
                g |= m & (keep | int(rng.integers(0, 1 << 62)))
        if g not in kinds:
            kinds.append(g)
    return kinds[:K]


def gres_wide_case(seed: int, N: int = 96, J: int = 700, P: int = 2, running: int = 60, layout: str | int = "uneven",
                   types: int | None = None, lists: bool = True, exclusive: bool = True):
    """(cluster, jobs, now, running) like tests.helpers.random_case, over a wide GRES layout (LAYOUTS, or an int: random_layout).

    types: the number of distinct res_total records of the snapshot (<= 64); 64 gives node type ids 0..63 (N >= 64: the first 64
    nodes take one record each, all schedulable)."""
    rng = np.random.default_rng(31_000 + seed)
    lay = make_layout(layout)
    cm = class_masks(lay)
    core_kinds = np.array([16, 32, 64, 128])
    if types is None:
        K = int(rng.integers(6, 13))
        combos = [(c, g) for c in range(4) for g in range(K)]
        pick = rng.choice(len(combos), min(len(combos), int(rng.integers(12, 40))), replace=False)
        combos = [combos[i] for i in sorted(pick)]
    else:
        assert types <= abi.MAX_NODE_TYPES and N >= types
        K = (types + 3) // 4
        combos = [(c, g) for g in range(K) for c in range(4)][:types]
    gk = _gres_kinds(lay, rng, K)
    K = len(gk)
    combos = [(c, g) for c, g in combos if g < K]
    ci = rng.integers(0, len(combos), N)
    if types is not None:
        assert len(combos) == types, "not enough distinct slot masks for the asked number of types"
        ci[:types] = np.arange(types)
    kind_c = np.array([combos[i][0] for i in ci])
    kind_g = np.array([combos[i][1] for i in ci])
    cores = core_kinds[kind_c]
    cpu_total_raw = (cores * 256).astype(np.int64)
    mem_total = cores.astype(np.uint64) * np.uint64(4 * GIB)
    core_lo = np.where(cores >= 64, np.uint64(M64), (np.uint64(1) << np.minimum(cores, 63).astype(np.uint64)) - np.uint64(1)).astype(np.uint64)
    core_hi = np.where(cores == 128, np.uint64(M64), np.uint64(0)).astype(np.uint64)
    gres_slots = np.array([gk[g] for g in kind_g], np.uint64)
    sched = (rng.random(N) > 0.04).astype(np.uint8)
    if types is not None:
        sched[:types] = 1
    part_lists = [np.nonzero(np.arange(N) % P == p)[0] for p in range(P)]
    part_offsets = np.cumsum([0] + [len(x) for x in part_lists]).astype(np.uint32)
    part_nodes = np.concatenate(part_lists).astype(np.uint32)
    cluster = abi.Cluster(cpu_total_raw, mem_total, core_lo, core_hi, gres_slots, part_offsets, part_nodes, gres=lay,
                          schedulable=sched)
    now = synth.NOW

    # running jobs: one node each, a few cores and a slice of the node's big classes, so that front counts cross 15 / 16 as they end
    run = None
    if running:
        free_g = [int(x) for x in gres_slots]
        seen = {}
        end, node, cpu, mem, lo, g = [], [], [], [], [], []
        for i in range(running):
            n = int(rng.integers(0, N))
            k = seen.get(n, 0)
            nc = int(rng.integers(1, 4))
            if 4 * k + 4 > cores[n]:
                continue
            seen[n] = k + 1
            take = 0
            for m in cm:
                avail = free_g[n] & m
                cnt = bin(avail).count("1")
                if cnt and rng.random() < 0.6:
                    want = int(rng.integers(1, cnt + 1)) if rng.random() < 0.5 else max(1, cnt // int(rng.integers(2, 5)))
                    bits = [b for b in range(64) if (avail >> b) & 1]
                    for b in rng.choice(bits, want, replace=False):
                        take |= 1 << int(b)
            free_g[n] &= ~take
            end.append(now + int(rng.integers(-50, 6000)))
            node.append(n); cpu.append(nc * 256); mem.append(nc * GIB)
            lo.append((((1 << nc) - 1) << (4 * k)) & M64); g.append(take)
        R = len(end)
        run = abi.Running(end_sec=end, alloc_offsets=np.arange(R + 1), alloc_node=node, alloc_cpu_raw=cpu, alloc_mem=mem,
                          alloc_core_lo=lo, alloc_core_hi=np.zeros(R, np.uint64), alloc_gres=np.array(g, np.uint64))

    # jobs
    k = np.where(rng.random(J) < 0.75, 1, rng.integers(1, 5, J)).astype(np.uint32)
    extra = np.where(rng.random(J) < 0.25, rng.integers(0, 5, J), 0).astype(np.uint32)
    ntasks = k + extra
    tmax = np.where(rng.random(J) < 0.3, rng.integers(1, 4, J), ntasks - k + 1).astype(np.int64)
    tmax = np.minimum(tmax, ntasks - k + 1)
    tmin = np.maximum(1, ntasks.astype(np.int64) - (k.astype(np.int64) - 1) * tmax)
    tmax = np.minimum(tmax, ntasks.astype(np.int64) - (k.astype(np.int64) - 1) * tmin)
    bad = tmin > tmax
    ntasks = np.where(bad, k, ntasks).astype(np.uint32)
    tmin = np.where(bad, 1, tmin).astype(np.uint32)
    tmax = np.where(bad, 1, tmax).astype(np.uint32)
    cpus = rng.choice([1, 2, 4, 8], J)
    task_cpu_raw = (cpus * 256).astype(np.int64)
    task_cpu_raw = np.where(rng.random(J) < 0.1, task_cpu_raw // 2 + 128, task_cpu_raw).astype(np.int64)
    task_mem = cpus.astype(np.uint64) * np.uint64(2 * GIB)
    L = (60 * rng.integers(1, 200, J)).astype(np.int64)
    partition = rng.integers(0, P, J).astype(np.uint32)
    partition = np.where(rng.random(J) < 0.01, P + 3, partition).astype(np.uint32)

    C, names = len(lay.class_name), sorted(set(lay.class_name))
    of_name = {a: [c for c in range(C) if lay.class_name[c] == a] for a in names}
    name_w = {a: sum(lay.class_width[c] for c in of_name[a]) for a in names}
    edge = lambda w: [14, 15, 16, 17, w, w + 1, 64, 65]
    gt = np.zeros((J, abi.MAX_GRES_NAMES), np.int64)
    gs = np.zeros((J, abi.MAX_GRES_CLASSES), np.int64)
    for j in range(J):
        s = int(rng.integers(0, 14))
        a = int(rng.choice(names))
        c = int(rng.choice(of_name[a]))
        w = lay.class_width[c]
        small = lambda hi: int(rng.integers(1, max(2, hi + 1)))
        if s <= 2:                                   # nothing
            continue
        if s == 3:                                   # untyped, moderate: spans several classes of a name
            gt[j, a] = small(min(name_w[a], 20))
        elif s == 4:                                 # untyped at the edges
            gt[j, a] = int(rng.choice(edge(name_w[a]) + [name_w[a] - 1, 18]))
        elif s == 5:                                 # typed, moderate; total = the typed count
            gs[j, c] = small(min(w, 18)); gt[j, a] = gs[j, c]
        elif s == 6:                                 # typed at the edges; total = the typed count
            gs[j, c] = int(rng.choice(edge(w) + [max(1, w - 1)])); gt[j, a] = gs[j, c]
        elif s == 7:                                 # typed + untyped rest of the same name (total above the typed sum)
            gs[j, c] = small(min(w, 16)); gt[j, a] = gs[j, c] + small(max(1, name_w[a] - gs[j, c]))
        elif s == 8:                                 # typed only (no total)
            gs[j, c] = small(min(w, 20))
        elif s == 9:                                 # bytes that cannot be met: 127, 128, 255
            v = int(rng.choice([127, 128, 255]))
            if rng.random() < 0.5:
                gs[j, c] = v; gt[j, a] = v
            else:
                gt[j, a] = v
        elif s == 10:                                # two classes of one name (if it has two) and a total above their sum
            cc = of_name[a][:2]
            for x in cc:
                gs[j, x] = small(min(lay.class_width[x], 12))
            gt[j, a] = int(gs[j].sum()) + int(rng.integers(0, 4))
        elif s == 11:                                # several names at once, one of them typed
            for b in names:
                if rng.random() < 0.7:
                    gt[j, b] = small(min(name_w[b], 17))
            gs[j, c] = min(int(gt[j, a]) if gt[j, a] else 1, w)
            gt[j, a] = max(int(gt[j, a]), int(gs[j, c]))
        elif s == 12:                                # a total below the typed count (the total adds nothing)
            gs[j, c] = small(min(w, 17)); gt[j, a] = max(1, int(gs[j, c]) - int(rng.integers(0, 3)))
        else:                                        # typed on one name, untyped on another
            gs[j, c] = small(min(w, 16))
            b = int(rng.choice(names))
            gt[j, b] = max(int(gt[j, b]), small(min(name_w[b], 17)))
    gt = np.minimum(gt, 255).astype(np.uint8)
    gs = np.minimum(gs, 255).astype(np.uint8)
    excl = ((rng.random(J) < 0.06) & exclusive).astype(np.uint8)
    skip = (rng.random(J) < 0.01).astype(np.uint8)
    incl_off = [0]; incl = []; excl_off = [0]; exn = []
    for j in range(J):
        if lists and rng.random() < 0.05:
            incl += list(rng.choice(N, size=int(rng.integers(1, min(12, N))), replace=False))
        if lists and rng.random() < 0.05:
            exn += list(rng.choice(N, size=int(rng.integers(1, min(30, N))), replace=False))
        incl_off.append(len(incl)); excl_off.append(len(exn))
    jobs = abi.Jobs(partition=partition, time_limit_sec=L, node_mem=np.where(rng.random(J) < 0.2, GIB, 0).astype(np.uint64),
                    task_cpu_raw=task_cpu_raw, task_mem=task_mem, node_num=k, ntasks=ntasks, ntasks_per_node_min=tmin,
                    ntasks_per_node_max=tmax, exclusive=excl, gres_total=gt, gres_spec=gs,
                    incl_offsets=np.array(incl_off, np.uint64), incl_nodes=np.array(incl if incl else [0], np.uint32),
                    excl_offsets=np.array(excl_off, np.uint64), excl_nodes=np.array(exn if exn else [0], np.uint32), skip=skip)
    return cluster, jobs, now, run


def repartition(cluster: abi.Cluster, jobs: abi.Jobs, seed: int, kind: str = "all+subsets"):
    """The same nodes laid out in 4 partitions that share nodes (as tests.test_overlap.overlap_case does)."""
    rng = np.random.default_rng(5000 + seed)
    N = cluster.num_nodes
    if kind == "all+subsets":
        parts = [np.arange(N - 8), np.sort(rng.choice(N - 8, (N - 8) // 3, replace=False)),
                 np.sort(rng.choice(N - 8, (N - 8) // 4, replace=False)), np.arange(N - 8, N)]
    elif kind == "chain":
        a, b = N // 4, N // 2
        parts = [np.arange(0, a + 4), np.arange(a - 4, b + 4), np.arange(b - 4, 3 * N // 4), np.arange(3 * N // 4, N)]
    else:
        parts = [np.nonzero(rng.random(N) < 0.45)[0] for _ in range(4)]
    off = np.cumsum([0] + [len(p) for p in parts]).astype(np.uint32)
    c = abi.Cluster(cluster.cpu_total_raw, cluster.mem_total, cluster.core_lo, cluster.core_hi, cluster.gres_slots, off,
                    np.concatenate(parts).astype(np.uint32), gres=cluster.gres, schedulable=cluster.schedulable)
    jobs.partition[:] = np.where(jobs.partition >= cluster.num_partitions, 7, rng.integers(0, 4, jobs.num_jobs)).astype(np.uint32)
    return c, jobs


def preempt_case(seed: int, N: int = 12, J: int = 80, P: int = 1, running: int = 24, layout: str | int = "uneven", nq: int = 3):
    """gres_wide_case + three QoS levels (2 may preempt 1 and 0, 1 may preempt 0), as tests.test_preempt.random_preempt_case; the
    running jobs hold big-class slots, so a preemption releases 16 and more slots of a class at once."""
    c, j, now, run = gres_wide_case(seed, N=N, J=J, P=P, running=running, layout=layout)
    rng = np.random.default_rng(seed * 7919 + 13)
    R = len(run.end_sec)
    rn_qos = rng.integers(0, nq, R)
    pd_qos = rng.integers(0, nq, j.num_jobs)
    qprio = np.array([10, 20, 30])
    rn_start = now - 1 - rng.permutation(R) * 7
    pd_prio = rng.permutation(j.num_jobs).astype(np.float64) + 0.5
    preempting = [int(1000 + r) for r in range(R) if rng.random() < 0.15] + [4242]
    pre = abi.Preempt([[], [0], [1, 0]][:nq], np.arange(j.num_jobs) + 1, pd_qos, qprio[pd_qos], pd_prio,
                      1000 + np.arange(R), rn_qos, qprio[rn_qos], rn_start, preempting=preempting)
    return c, j, now, run, pre


def resv_case(seed: int, N: int = 48, J: int = 500, V: int = 6, layout: str | int = "uneven"):
    """gres_wide_case + reservations (active / future / expired) that hold cores AND big-class GRES slots, as
    tests.test_reservations.random_resv_case; a quarter of the jobs run inside one (or name an unknown one)."""
    c, j, now, run = gres_wide_case(seed, N=N, J=J, P=2, running=0, layout=layout, lists=False)
    rng = np.random.default_rng(4242 + seed)
    st, en, off, node, cpu, mem, lo, g = [], [], [0], [], [], [], [], []
    for v in range(V):
        kind = v % 3
        if kind == 0: s, e = now - int(rng.integers(1, 500)), now + int(rng.integers(2000, 9000))
        elif kind == 1: s = now + int(rng.integers(100, 4000)); e = s + int(rng.integers(500, 5000))
        else: s, e = now - 5000, now - int(rng.integers(1, 100))
        st.append(s); en.append(e)
        for n in rng.choice(N, size=int(rng.integers(2, 8)), replace=False):
            cores = int(c.cpu_total_raw[n] // 256)
            take = int(rng.integers(1, max(2, cores // 4)))
            first = int(rng.integers(0, min(cores, 64) - take + 1))
            slots = int(c.gres_slots[n])
            keep = slots & (int(rng.integers(0, 1 << 62)) | (int(rng.integers(0, 4)) << 62)) if rng.random() < 0.7 else 0
            node.append(int(n)); cpu.append(take * 256); mem.append(take * GIB); lo.append(((1 << take) - 1) << first)
            g.append(keep)
        off.append(len(node))
    rv = abi.Reservations(st, en, off, node, cpu, mem, lo, np.zeros(len(node), np.uint64), np.array(g, np.uint64))
    resv = np.full(j.num_jobs, abi.RESV_NONE, np.uint32)
    pick = rng.random(j.num_jobs) < 0.25
    resv[pick] = rng.integers(0, V + 1, int(pick.sum()))
    j.reservation = resv
    return c, j, now, None, rv


def step_case(seed: int, layout: str | int = "uneven", J: int = 300):
    """StepJobs / Steps (include/crane_gpu/steps.h) whose nodes hold wide GRES: each job's nodes carry full, partial or empty slot
    masks of the layout, the steps ask per node for counts around 15 / 16 / the class width, typed and untyped, on every name."""
    from cranesched_amd import steps as st
    rng = np.random.default_rng(seed + 6100)
    lay = make_layout(layout)
    kinds = _gres_kinds(lay, rng, 12)
    C, names = len(lay.class_name), sorted(set(lay.class_name))
    of_name = {a: [c for c in range(C) if lay.class_name[c] == a] for a in names}
    off, idx, cpu, mem, lo, gg, nsteps = [0], [], [], [], [], [], []
    for _ in range(J):
        k = int(rng.integers(1, 5))
        for n in sorted(rng.choice(500, k, replace=False).tolist()):
            cores = int(rng.integers(0, 1 << 16)) | (int(rng.integers(0, 2)) << 16)
            idx.append(n); cpu.append(bin(cores).count("1") * 256 + int(rng.integers(0, 3)) * 64)
            mem.append(int(rng.integers(1, 64)) * GIB); lo.append(cores); gg.append(kinds[int(rng.integers(0, len(kinds)))])
        off.append(len(idx))
        nsteps.append(int(rng.integers(1, 5)))
    jobs = st.StepJobs(off, idx, cpu, mem, lo, [0] * len(lo), gg, np.cumsum([0] + nsteps))
    S = int(sum(nsteps))
    spec = dict(node_cpu_raw=[], node_mem=[], task_cpu_raw=[], task_mem=[], node_num=[], ntasks=[], tmin=[], tmax=[])
    io, inn, eo, enn = [0], [], [0], []
    for j in range(J):
        nodes = idx[off[j]:off[j + 1]]
        for _ in range(nsteps[j]):
            kk = int(rng.integers(1, min(len(nodes), 3) + 1))
            tmax = int(rng.integers(1, 4))
            tmin = int(rng.integers(1, tmax + 1))
            spec["node_num"].append(kk); spec["ntasks"].append(kk + int(rng.integers(0, 4)))
            spec["tmin"].append(tmin); spec["tmax"].append(tmax)
            spec["task_cpu_raw"].append(int(rng.choice([128, 256, 256, 512]))); spec["task_mem"].append(int(rng.integers(0, 4)) * GIB)
            spec["node_cpu_raw"].append(0); spec["node_mem"].append(0)
            if rng.random() < 0.15:
                inn += rng.choice(nodes, int(rng.integers(1, len(nodes) + 1)), replace=False).tolist()
            if rng.random() < 0.1:
                enn += rng.choice(nodes, 1).tolist()
            io.append(len(inn)); eo.append(len(enn))
    steps = st.Steps(node_cpu_raw=spec["node_cpu_raw"], node_mem=spec["node_mem"], task_cpu_raw=spec["task_cpu_raw"],
                     task_mem=spec["task_mem"], node_num=spec["node_num"], ntasks=spec["ntasks"], tmin=spec["tmin"],
                     tmax=spec["tmax"], incl_offsets=io, incl_nodes=inn or [0], excl_offsets=eo, excl_nodes=enn or [0])
    gt, gs = np.zeros((S, 4), np.uint8), np.zeros((S, 8), np.uint8)
    for s in range(S):
        a = int(rng.choice(names)); c = int(rng.choice(of_name[a])); w = lay.class_width[c]
        sel = int(rng.integers(0, 7))
        if sel == 0: gt[s, a] = rng.integers(1, 5)
        elif sel == 1: gt[s, a] = rng.choice([14, 15, 16, 17, min(255, sum(lay.class_width[x] for x in of_name[a]))])
        elif sel == 2: v = int(rng.choice([1, 2, 14, 15, 16, 17, w, w + 1])); gs[s, c] = v; gt[s, a] = v
        elif sel == 3: v = int(rng.integers(1, min(w, 16) + 1)); gs[s, c] = v; gt[s, a] = v + int(rng.integers(1, 6))
        elif sel == 4:
            for b in names:
                gt[s, b] = rng.integers(0, 4)
    steps.node_gres_total, steps.node_gres_spec = gt, gs
    return lay, jobs, steps


def probe_case(seed: int, layout: str | int, Q: int = 32):
    """(cluster, jobs, probes, now, running) for cns_probe: gres_wide_case(seed)'s cycle, and as probes the first Q jobs of the queue of
    gres_wide_case(1000 + seed) on the same layout (the queue depends on the layout, N and P only, so the probes fit the cluster)."""
    from tests import probe_case as pc
    c, j, now, run = gres_wide_case(seed, N=96, J=700, P=2, running=60, layout=layout)
    p = gres_wide_case(1000 + seed, N=96, J=700, P=2, running=0, layout=layout)[1]
    return c, j, pc.take(p, np.arange(Q)), now, run


def probe_dip_kat(kind: str):
    """Hand-made, on one64: probes whose window reaches a slot's dip (KParams::dip_*: the packed bounds of a FUTURE time-map entry below
    the front, 4 bits per class) where the dip's class count saturates.
    -> (cluster, jobs, reservations, probes, now, the free slots of node 0 over time, [(start, node) per probe])

    Node 0 has 64 slots, node 1 the low 20.  Job 0 takes 30 slots of node 0 for 600 s.  Job 1 (32 of 64 cores, 6 000 s) goes to the
    then cheaper node 1 and makes it the dearer one.  From now + 600 to now + 1 200 node 0 has 24 free slots — below the front's 34,
    above the 15 a nibble can say — and the engine holds that entry as the slot's dip:
      "reservation": a reservation of the low 40 slots over that time (the dip the snapshot's initialisation records; job 0 holds the
                     low 30 slots and is gone by then, so slots 40..63 are free throughout);
      "backfill":    job 2 asks for 40 slots, which only node 0 has, and is backfilled behind job 0; job 3 asks for 30 slots for
                     3 600 s: the front admits it, the entry at now + 600 does not (the dip the cycle records where its prediction
                     fails), and it starts at now + 1 200.
    Probes of 3 600 s: 17 slots typed and 17 untyped start now on node 0, the cheaper node (17 <= 24 at the dip); a filter that read
    the saturated 15 as exact would send them to node 1 (20 free).  25 slots for 300 s end before the dip and start now on node 0."""
    from tests import kat
    lay = make_layout("one64")
    now = synth.NOW
    c = kat.cluster([64, 64], mem_gib=[256, 256], gres=[M64, (1 << 20) - 1], layout=lay)
    specs = [dict(L=600, gspec=[30]), dict(cpu=32, L=6000)]
    rv = None
    if kind == "reservation":
        rv = abi.Reservations([now + 600], [now + 1200], [0, 1], [0], [256], [GIB], [1 << 63], [0], [(1 << 40) - 1])
        free = [(now, 34), (now + 600, 24), (now + 1200, 64)]
    else:
        specs += [dict(L=600, gspec=[40]), dict(L=3600, gspec=[30])]
        free = [(now, 34), (now + 600, 24), (now + 1200, 34), (now + 4800, 64)]
    probes = kat.jobs([dict(L=3600, gspec=[17]), dict(L=3600, gtot=[17]), dict(L=300, gspec=[25])])
    return c, kat.jobs(specs), rv, probes, now, free, [(now, 0), (now, 0), (now, 0)]


DIP_KATS = ("reservation", "backfill")
SUBMIT_COUNT_CAP = 12  # the count bytes of submit_case's jobs: uncapped (127, 255, x node_num) nearly every job fails :111-114


def submit_case(seed: int, layout: str | int, J: int = 600):
    """(SubmitTables, jobs, SubmitKeys) for cns_check_submissions over a wide layout: 40 users, 12 accounts in two trees of depth <= 4,
    4 QoS with deny_on_limit alternating, 3 partitions, 4 partition limits.  Every TRES limit is drawn as
    tests.test_run_limits.random_limit_case.rtres draws it, over every name and class of the layout (a name present with probability
    0.6, a class with 0.5), so that limits lack names and classes the jobs ask for: CheckGres_'s early `return true` (:1034, :1044) at
    the first entry a limit lacks makes the walk order (ascending name, its total, its classes ascending) decide codes.  The usage of
    the (user, qos) and (account, qos) records has counts on every class.  node_num, ntasks and the GRES bytes of the jobs are those of
    gres_wide_case's queue, the bytes capped at SUBMIT_COUNT_CAP."""
    from cranesched_amd import limits as lm, submit as sb
    rng = np.random.default_rng(52_000 + seed)
    lay = make_layout(layout)
    nc, names = len(lay.class_name), sorted(set(lay.class_name))
    U, A, Q, Pn = 40, 12, 4, 3
    NONE = sb.LIM_NONE
    # two trees: 0 <- 1 <- 2 <- 3 (depth 4), 0 <- 4, 1 <- 5; 6 <- 7 <- 8, 6 <- 9, 7 <- 10, 6 <- 11
    parent = np.array([NONE, 0, 1, 2, 0, 1, NONE, 6, 7, 6, 7, 6], np.uint32)

    def rtres(scale):
        if rng.random() < 0.2:
            return lm.unlimited_tres()
        nm = {int(n): int(rng.integers(1, 6 * scale + 1)) for n in names if rng.random() < 0.6}
        cl = {int(g): int(rng.integers(1, 4 * scale + 1)) for g in range(nc) if rng.random() < 0.5}
        return lm.tres(cpu=int(rng.integers(64, 512)) if rng.random() < 0.3 else None, names=nm, classes=cl)

    qos = [sb.submit_qos(deny_on_limit=bool(q % 2), max_submit_jobs_per_user=int(rng.integers(20, 60)) if q == 1 else lm.UNLIMITED_JOBS,
                         max_tres=rtres(40), max_tres_per_user=rtres(12), max_tres_per_account=rtres(8)) for q in range(Q)]
    pl = [sb.submit_part_limit(max_tres_per_job=rtres(8)) for _ in range(4)]
    upl = np.where(rng.random(U * Pn) < 0.4, rng.integers(0, len(pl), U * Pn), NONE).astype(np.uint32)
    apl = np.where(rng.random(A * Pn) < 0.3, rng.integers(0, len(pl), A * Pn), NONE).astype(np.uint32)

    def rusage(n, hi):
        u = np.zeros(n, lm.USAGE_DT)
        u["cpu_raw"] = rng.integers(0, 16, n) * 256
        for g in range(nc):
            c = rng.integers(0, hi, n)
            u["class_count"][:, g] = c
            u["name_total"][:, lay.class_name[g]] += c.astype(np.uint64)
        for a in names:                                           # ... and an untyped part on top of some totals
            u["name_total"][:, a] += np.where(rng.random(n) < 0.3, rng.integers(0, 4, n), 0).astype(np.uint64)
        return u

    t = sb.SubmitTables(layout=lay, num_users=U, num_user_accts=U, num_partitions=Pn, qos=np.array(qos), acct_parent=parent,
                        part_limits=np.array(pl), user_part_limit=upl, acct_part_limit=apl, user_qos=rusage(U * Q, 5), acct_qos=rusage(A * Q, 13),
                        qos_usage=rusage(Q, 13), user_qos_submit=rng.integers(0, 3, U * Q), user_part_submit=rng.integers(0, 3, U * Pn),
                        acct_qos_submit=rng.integers(0, 5, A * Q), acct_part_submit=rng.integers(0, 5, A * Pn), qos_submit=rng.integers(0, 9, Q),
                        user_exists=rng.random(U) < 0.7, acct_exists=rng.random(A) < 0.7, qos_exists=rng.random(Q) < 0.75)
    q = gres_wide_case(seed, N=96, J=J, P=2, running=0, layout=layout)[1]
    jobs = abi.Jobs(partition=rng.integers(0, Pn, J).astype(np.uint32), time_limit_sec=q.time_limit_sec, node_mem=q.node_mem,
                    task_cpu_raw=q.task_cpu_raw, task_mem=q.task_mem, node_num=q.node_num, ntasks=q.ntasks,
                    ntasks_per_node_min=q.ntasks_per_node_min, ntasks_per_node_max=q.ntasks_per_node_max,
                    gres_total=np.minimum(q.gres_total, SUBMIT_COUNT_CAP).astype(np.uint8),
                    gres_spec=np.minimum(q.gres_spec, SUBMIT_COUNT_CAP).astype(np.uint8))
    user = rng.integers(0, U, J).astype(np.uint32)
    ua_acct = rng.integers(0, A, U).astype(np.uint32)              # user_acct i = (user i, account ua_acct[i])
    count = np.where(rng.random(J) < 0.05, rng.integers(2, 4, J), 1).astype(np.uint32)
    keys = sb.SubmitKeys(user, user.copy(), ua_acct[user], rng.integers(0, Q, J), count, (rng.random(J) < 0.02).astype(np.uint8))
    return t, jobs, keys


def with_sorted_class_names(t):
    """The same SubmitTables over the layout whose class_name is sorted: there class-index order IS name order, so the jobs whose code
    changes are jobs on which the two walk orders part."""
    import dataclasses
    lay = t.layout
    return dataclasses.replace(t, layout=abi.GresLayout(class_name=sorted(lay.class_name), class_shift=list(lay.class_shift),
                                                        class_width=list(lay.class_width)))


def wide_case_of(layout: str | int):
    """gres_wide_case over `layout` with tests.helpers.random_case's signature (tests.running_case.scenario's `case`)."""
    def case(seed, N=96, J=600, P=2, running=40):
        return gres_wide_case(seed, N=N, J=J, P=P, running=running, layout=layout)
    return case


# ---------------------------------------------------------------------------------------------------------------------------------
# coverage: what the oracle's own placements show a case reaches
# ---------------------------------------------------------------------------------------------------------------------------------
def coverage(cluster: abi.Cluster, jobs: abi.Jobs, pl: abi.Placements) -> dict:
    """Facts about one cycle's result: the largest number of slots of one class a start-now placement took, whether any placement holds
    bit 63, which names were allocated, exclusive starts on nodes with a class of >= 16 slots, backfilled / refused counts."""
    lay = cluster.gres
    cm = class_masks(lay)
    J = jobs.num_jobs
    r = pl.reason[:J]
    off = pl.place_offsets
    big_node = np.array([max([0] + class_counts(lay, int(g))) >= 16 for g in cluster.gres_slots])
    out = dict(max_class_now=0, bit63=False, names=set(), excl_big_now=0, backfilled=int((r == abi.REASON_PRIORITY).sum()),
               started=int((r == abi.REASON_NONE).sum()), resource=int((r == abi.REASON_RESOURCE).sum()), gres_jobs_now=0)
    for j in range(J):
        if r[j] not in (abi.REASON_NONE, abi.REASON_PRIORITY):
            continue
        any_g = False
        for p in range(int(off[j]), int(off[j + 1])):
            g = int(pl.gres[p])
            if not g:
                continue
            any_g = True
            out["bit63"] |= bool(g >> 63)
            for c, m in enumerate(cm):
                if g & m:
                    out["names"].add(lay.class_name[c])
                    if r[j] == abi.REASON_NONE:
                        out["max_class_now"] = max(out["max_class_now"], bin(g & m).count("1"))
            if r[j] == abi.REASON_NONE and jobs.exclusive[j] and big_node[int(pl.node_idx[p])]:
                out["excl_big_now"] += 1
        out["gres_jobs_now"] += int(any_g and r[j] == abi.REASON_NONE)
    return out


def num_types(cluster: abi.Cluster) -> int:
    """Distinct res_total records among the schedulable nodes that some partition lists."""
    listed = np.zeros(cluster.num_nodes, bool)
    listed[np.asarray(cluster.part_nodes, np.int64)] = True
    if cluster.schedulable is not None:
        listed &= cluster.schedulable != 0
    recs = {(int(cluster.cpu_total_raw[n]), int(cluster.mem_total[n]), int(cluster.core_lo[n]), int(cluster.core_hi[n]),
             int(cluster.gres_slots[n])) for n in np.nonzero(listed)[0]}
    return len(recs)
