"""Cases that put the run-limit admission (include/crane_gpu/run_limits.h, csrc/limits_kernels.hip) on the seams of its device code:
item chunks, the carry's row groups, a chunk length that is no multiple of the load batch, the block scan past one block count per
thread, account chains of every length, more than 65 536 usage records.  Plain numpy, usable without a GPU; the sizes come from
`shape()` (cns_limits_shape), never from a number typed in here.

Every generator returns a `Case`: a flat cluster (n x 64 cores, one NodeSelect partition, tests.helpers.multi_type_layout) and jobs
of one core, 100 s and 16 MiB, so that every intended candidate starts now and the "unlimited" memory cap of a default TRES
(CNS_LIM_MAX_JOB_MEMORY, about 10 TiB) stays far away: 40 000 admitted jobs hold 625 GiB.

A candidate whose account sits on tree level L holds 5 + 2 L usage records (user x qos, user x partition, the QoS globally, two per
account of its chain): `n_items`.

`scalar_items` + `bracket_rounds` are the numpy form of tests/test_device_logic_models.py::bracketing with several records per job:
they say how many rounds the parallel pass needs, so that "no ordered fallback" is a property of the case."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from cranesched_amd import abi, limits as lm
from tests import helpers, kat

NONE = lm.LIM_NONE
MIB = 1 << 20
JOB_MEM = 16 * MIB
JOB_L = 100
NODE_CORES = 64
NOW = kat.NOW
CHAIN = [NONE, 0, 1, 2, 3, 4]          # account a = tree level a


@dataclass
class Case:
    cluster: abi.Cluster
    jobs: abi.Jobs
    now: int
    lay: abi.GresLayout
    t: lm.LimitTables
    lj: lm.LimitJobs
    info: dict


def shape():
    """cns_limits_shape without a handle: (min_item_chunk, num_chunks, batch, carry_row_chunks, max_rounds, scan_jobs)"""
    from cranesched_amd import engine
    v = [C.c_uint32(0) for _ in range(6)]
    assert engine.lib().cns_limits_shape(*[C.byref(x) for x in v]) == 0
    return tuple(x.value for x in v)


def n_items(levels) -> int:
    return int(sum(5 + 2 * int(l) for l in levels))


def flat_cluster(cores_needed: int):
    lay = helpers.multi_type_layout()
    n = max(1, -(-int(cores_needed) // NODE_CORES))
    return kat.cluster([NODE_CORES] * n, mem_gib=[16] * n, layout=lay), lay


def one_core_jobs(cores) -> abi.Jobs:
    """cores[j] whole cores per job (1: starts now on the flat cluster; NODE_CORES + 1: fits no node, stays pending)"""
    cores = np.asarray(cores, np.int64)
    J = len(cores)
    one = np.ones(J, np.uint32)
    return abi.Jobs(partition=np.zeros(J, np.uint32), time_limit_sec=np.full(J, JOB_L, np.int64), node_mem=np.zeros(J, np.uint64),
                    task_cpu_raw=cores * 256, task_mem=np.full(J, JOB_MEM, np.uint64), node_num=one, ntasks=one,
                    ntasks_per_node_min=one, ntasks_per_node_max=one, exclusive=np.zeros(J, np.uint8),
                    gres_total=np.zeros((J, abi.MAX_GRES_NAMES), np.uint8), gres_spec=np.zeros((J, abi.MAX_GRES_CLASSES), np.uint8))


def _case(t, lj, info, cores=None):
    cores = np.ones(lj.num_jobs, np.int64) if cores is None else np.asarray(cores, np.int64)
    cluster, lay = flat_cluster(int(cores[cores <= NODE_CORES].sum()))
    return Case(cluster, one_core_jobs(cores), NOW, lay, t, lj, info)


# ---- hot: every record one segment ---------------------------------------------------------------------------------------
def hot_split(items: int, level: int):
    """(a, level, b, other level) with a (5 + 2 level) + b (5 + 2 other) == items, b as small as possible"""
    p = 5 + 2 * level
    other = level + 1 if level < 5 else level - 1
    q = 5 + 2 * other
    for b in range(p):
        if items - q * b >= 0 and (items - q * b) % p == 0:
            return (items - q * b) // p, level, b, other
    raise ValueError(f"{items} items cannot be made of candidates with {p} and {q} items")


def hot(items: int, level: int = 0) -> Case:
    """One user, one QoS, account `level` of one chain (a few candidates one level beside it where `items` is no multiple of
    5 + 2 level; they sit in the second half of the queue).  Four limit partitions, job i in partition i % 4:
      p0: a wall limit on the leaf account x p0      -> AccPartitionWallTimeLimit past M / 16 admitted (a quarter of the queue in)
      p1: a wall limit on the root account x p1      -> AccPartitionWallTimeLimit past M / 8  (half of the queue in)
      p2: a job limit on the (user, account) x p2    -> UserPartitionJobsLimit    past M / 12 (a third of the queue in)
      p3: none
    and one cap of the QoS that ends the admission for everybody at T = 0.44 M admitted jobs (two thirds of the queue in); which one rotates with `items`:
    max_jobs, max_jobs_per_account, max_cpus_per_user, the per-account cpu TRES.  The other three sit 1, 2 and 3 above T: a sum
    that is a few too high anywhere flips a reason."""
    a, la, b, lb = hot_split(items, level)
    M = a + b
    assert M >= 8, "too few candidates for caps in the middle"
    lv = np.full(M, la, np.uint32)
    if b:
        lv[M // 2 + (M // 2) // b * np.arange(b)] = lb
    assert n_items(lv) == items
    Mq = M // 4
    kA, kB, kC, T = max(1, Mq // 4), max(1, Mq // 2), max(1, Mq // 3), max(6, 44 * M // 100)
    caps = [T + 1, T + 2, T + 3, T + 4]
    caps[(items + items // 64) % 4] = T
    qos = [lm.qos_limits(max_jobs=caps[0], max_jobs_per_account=caps[1], max_cpus_per_user=caps[2],
                         max_tres_per_account=lm.tres(cpu=caps[3]))]
    pls = np.array([lm.part_limit(max_wall_sec=JOB_L * kA), lm.part_limit(max_wall_sec=JOB_L * kB), lm.part_limit(max_jobs=kC)],
                   lm.PART_LIMIT_DT)
    A, Pn = len(CHAIN), 4
    apl = np.full(A * Pn, NONE, np.uint32)
    apl[la * Pn + 0] = 0
    apl[0 * Pn + 1] = 1
    upl = np.full(A * Pn, NONE, np.uint32)        # user_acct x = (user 0, account x)
    upl[np.arange(A) * Pn + 2] = 2
    t = lm.LimitTables(num_users=1, num_user_accts=A, num_partitions=Pn, qos=np.array(qos, lm.QOS_DT),
                       acct_parent=np.array(CHAIN, np.uint32), part_limits=pls, user_part_limit=upl, acct_part_limit=apl)
    z = np.zeros(M, np.uint32)
    lj = lm.LimitJobs(user=z, user_acct=lv, account=lv, qos=z, partition=np.arange(M) % Pn, time_limit_sec=np.full(M, JOB_L, np.int64))
    return _case(t, lj, dict(levels=lv, items=items, candidates=M))


# ---- a segment that starts on the last item in front of a boundary ---------------------------------------------------------
def segment_on_last_item(boundary: int) -> Case:
    """User 0 holds boundary - 1 candidates, user 1 three.  base_uq = 0: the user x qos records sort first, so the segment of user
    1's record starts on item boundary - 1 and goes on behind the boundary.  max_jobs_per_user = boundary + 1 and user 1 starts
    with boundary - 1 jobs: two of its three are admitted."""
    M = boundary - 1 + 3
    user = np.array([0] * (boundary - 1) + [1, 1, 1], np.uint32)
    uq = np.zeros(2, lm.USAGE_DT)
    uq["jobs_count"][1] = boundary - 1
    t = lm.LimitTables(num_users=2, num_user_accts=2, num_partitions=1, qos=np.array([lm.qos_limits(max_jobs_per_user=boundary + 1)], lm.QOS_DT),
                       acct_parent=np.array([NONE], np.uint32), user_qos=uq)
    z = np.zeros(M, np.uint32)
    lj = lm.LimitJobs(user=user, user_acct=user, account=z, qos=z, partition=z, time_limit_sec=np.full(M, JOB_L, np.int64))
    return _case(t, lj, dict(levels=z, items=5 * M, candidates=M, tail=[0, 0, 3]))


# ---- account chains of every length ------------------------------------------------------------------------------------------
DEEP_PARENT = CHAIN + [1, 6, 0, NONE, 9]     # + a branch a6 (level 2) - a7 (level 3) under a1, a8 under a0, a second root a9 - a10
DEEP_LEVEL = [0, 1, 2, 3, 4, 5, 2, 3, 1, 0, 1]


def deep_tree(seed: int, J: int = 1500) -> Case:
    """Random tables over a tree with chains of 1 to 6 accounts, jobs on accounts of every level, every second job on the two
    deepest.  Partition limits and tight per-account limits reach levels 4 and 5 (slots 11 - 14 of a job's record), some usage
    entries of the deep accounts are missing, and the job limits per account are so tight that a deep and a shallow account of
    one chain run full at once."""
    rng = np.random.default_rng(41000 + seed)
    A, U, Q, Pn = len(DEEP_PARENT), 6, 3, 2
    ua_pairs = [(u, a) for u in range(U) for a in range(A) if (u + a) % 2 == 0 or a >= 4]
    UA = len(ua_pairs)
    deep = [x for x, (_, a) in enumerate(ua_pairs) if DEEP_LEVEL[a] >= 4]

    def rtres(lo, hi):
        if rng.random() < 0.25:
            return lm.unlimited_tres()
        return lm.tres(cpu=int(rng.integers(lo, hi)) if rng.random() < 0.7 else None,
                       mem=int(rng.integers(lo, hi)) * JOB_MEM if rng.random() < 0.5 else None)

    qos = [lm.qos_limits(max_jobs_per_user=int(rng.integers(40, 120)) if rng.random() < 0.5 else lm.UNLIMITED_JOBS,
                         max_jobs_per_account=int(rng.integers(15, 60)) if q < 2 else lm.UNLIMITED_JOBS,
                         max_jobs=int(rng.integers(200, 400)) if rng.random() < 0.5 else lm.UNLIMITED_JOBS,
                         max_cpus_per_user=int(rng.integers(40, 150)) if rng.random() < 0.5 else None,
                         max_wall_sec=int(rng.integers(3000, 20000)) if q == 1 else 0,
                         max_tres=rtres(150, 500), max_tres_per_user=rtres(30, 120),
                         max_tres_per_account=rtres(12, 70) if q > 0 else lm.unlimited_tres())
           for q in range(Q)]
    pls = np.array([lm.part_limit(max_jobs=int(rng.integers(5, 40)) if rng.random() < 0.6 else lm.UNLIMITED_JOBS,
                                  max_wall_sec=int(rng.integers(500, 6000)) if rng.random() < 0.5 else 0,
                                  max_tres=rtres(8, 50)) for _ in range(6)], lm.PART_LIMIT_DT)
    pick = lambda n, p: np.where(rng.random(n) < p, rng.integers(0, len(pls), n), NONE).astype(np.uint32)
    apl = pick(A * Pn, 0.3)
    for a in (4, 5):                                   # the two deepest accounts carry a partition limit in both partitions
        apl[a * Pn:(a + 1) * Pn] = rng.integers(0, len(pls), Pn)

    def rusage(n, p=0.3):
        u = np.zeros(n, lm.USAGE_DT)
        on = rng.random(n) < p
        u["cpu_raw"] = np.where(on, rng.integers(0, 6, n) * 256, 0)
        u["mem"] = np.where(on, rng.integers(0, 6, n) * JOB_MEM, 0)
        u["wall_sec"] = np.where(on, rng.integers(0, 400, n), 0)
        u["jobs_count"] = np.where(on, rng.integers(0, 4, n), 0)
        return u

    aqe, ape = np.ones(A * Q, np.uint8), np.ones(A * Pn, np.uint8)
    aqe[4 * Q + 2] = 0                                 # (a4, qos 2): QosEntryNotFound for the jobs of a4 and a5 in that QoS
    ape[5 * Pn + 1] = 0                                # (a5, p1) has a limit and no entry: PartitionEntryNotFound
    ape[3 * Pn + 0] = 0                                # (a3, p0): no limit there -> the entry is created by the first admission
    apl[3 * Pn + 0] = NONE
    ape[7 * Pn:(8) * Pn] = 0
    t = lm.LimitTables(num_users=U, num_user_accts=UA, num_partitions=Pn, qos=np.array(qos, lm.QOS_DT),
                       acct_parent=np.array(DEEP_PARENT, np.uint32), part_limits=pls, user_part_limit=pick(UA * Pn, 0.3),
                       acct_part_limit=apl, user_qos=rusage(U * Q), user_part=rusage(UA * Pn), acct_qos=rusage(A * Q), acct_qos_exists=aqe,
                       acct_part=rusage(A * Pn), acct_part_exists=ape, qos_usage=rusage(Q, 1.0))
    uax = np.where(rng.random(J) < 0.5, rng.choice(deep, J), rng.integers(0, UA, J))
    order = rng.permutation(J).astype(np.uint64)
    lj = lm.LimitJobs(user=[ua_pairs[x][0] for x in uax], user_acct=uax, account=[ua_pairs[x][1] for x in uax],
                      qos=rng.choice(Q, J, p=[0.45, 0.2, 0.35]), partition=rng.integers(0, Pn, J),
                      time_limit_sec=np.full(J, JOB_L, np.int64), select_index=order, skip=(rng.random(J) < 0.02).astype(np.uint8))
    return _case(t, lj, dict(levels=np.array(DEEP_LEVEL)[lj.account]))


# ---- more than 65 536 usage records -------------------------------------------------------------------------------------------
def many_records(seed: int, J: int = 3000, U: int = 9000, Q: int = 8) -> Case:
    """U x Q user x qos records alone need 17 key bits: three 8-bit radix passes.  The candidates crowd on the lowest and the
    highest user indices (and a few between), so per-user caps bind on records below 256, above 65 536 and across the digit
    borders.  user_acct = user, account = user % 4 in a tree of two levels."""
    rng = np.random.default_rng(52000 + seed)
    assert U * Q >= 65536
    parent = [NONE, 0, 0, NONE]
    A, Pn = len(parent), 2
    qos = [lm.qos_limits(max_jobs_per_user=int(rng.integers(2, 7)), max_cpus_per_user=int(rng.integers(3, 9)) if q % 2 else None,
                         max_jobs_per_account=int(rng.integers(150, 400)) if q % 3 == 0 else lm.UNLIMITED_JOBS) for q in range(Q)]
    pls = np.array([lm.part_limit(max_jobs=3), lm.part_limit(max_wall_sec=4 * JOB_L)], lm.PART_LIMIT_DT)
    upl = np.where(rng.random(U * Pn) < 0.3, rng.integers(0, 2, U * Pn), NONE).astype(np.uint32)
    uqe = np.ones(U * Q, np.uint8)
    uqe[rng.integers(0, U * Q, 2000)] = 0
    uqe[(U - 3) * Q:(U - 2) * Q] = 0
    t = lm.LimitTables(num_users=U, num_user_accts=U, num_partitions=Pn, qos=np.array(qos, lm.QOS_DT), acct_parent=np.array(parent, np.uint32),
                       part_limits=pls, user_part_limit=upl, user_qos_exists=uqe)
    pool = np.concatenate([np.arange(40), np.arange(U - 40, U), 8192 // Q * np.arange(1, 9) + rng.integers(-2, 3, 8), rng.integers(0, U, 60)])
    user = rng.choice(pool, J).astype(np.uint32)
    lj = lm.LimitJobs(user=user, user_acct=user, account=user % A, qos=rng.integers(0, Q, J), partition=rng.integers(0, Pn, J),
                      time_limit_sec=np.full(J, JOB_L, np.int64), select_index=rng.permutation(J).astype(np.uint64),
                      skip=(rng.random(J) < 0.01).astype(np.uint8))
    return _case(t, lj, dict(levels=np.array([0, 1, 1, 0])[lj.account], records=U * Q + U * Pn + A * Q + A * Pn + Q))


# ---- few candidates in a long queue ----------------------------------------------------------------------------------------------
PATTERNS = ("lane63", "lane0", "alt_wave", "stride_lastblock", "none")


def candidate_mask(J: int, pattern: str) -> np.ndarray:
    i = np.arange(J)
    if pattern == "lane63":                 # only the last lane of every wave
        return i % 64 == 63
    if pattern == "lane0":
        return i % 64 == 0
    if pattern == "alt_wave":               # every second wave empty, the others hold one or two candidates on moving lanes
        w = i // 64
        return (w % 2 == 0) & ((i % 64 == (w * 7) % 64) | ((w % 6 == 0) & (i % 64 == 63 - (w * 3) % 64)))
    if pattern == "stride_lastblock":       # one candidate every 700 jobs + the whole last block of 256
        return (i % 700 == 0) | (i >= (max(J, 1) - 1) // 256 * 256)
    if pattern == "none":
        return np.zeros(J, bool)
    raise ValueError(pattern)


def sparse_candidates(J: int, pattern: str) -> Case:
    """J limit jobs, candidates where `candidate_mask` says.  The others: mostly jobs of NODE_CORES + 1 cores, which NodeSelect leaves
    pending; every 97th (all of them for pattern "none") a job that starts and has `skip` set.  select_index is a permutation."""
    rng = np.random.default_rng(63000 + J * 7 + PATTERNS.index(pattern))
    cand = candidate_mask(J, pattern)
    runs = cand | (np.arange(J) % 97 == 5) | (pattern == "none")
    skip = (runs & ~cand).astype(np.uint8)
    sel = rng.permutation(J).astype(np.uint64)
    cores = np.full(J, NODE_CORES + 1, np.int64)
    cores[sel[runs].astype(np.int64)] = 1
    parent = [NONE, 0, 1]
    U, A, Q, Pn = 5, len(parent), 2, 1
    M = int(cand.sum())
    qos = [lm.qos_limits(max_jobs_per_user=max(1, M // 12)), lm.qos_limits(max_cpus_per_user=max(1, M // 15), max_jobs_per_account=max(1, M // 4))]
    t = lm.LimitTables(num_users=U, num_user_accts=U * A, num_partitions=Pn, qos=np.array(qos, lm.QOS_DT), acct_parent=np.array(parent, np.uint32))
    user = rng.choice(U, J, p=[0.4, 0.15, 0.15, 0.15, 0.15]).astype(np.uint32)      # user 0 reaches its cpu cap before the accounts fill
    acct = rng.integers(0, A, J).astype(np.uint32)
    lj = lm.LimitJobs(user=user, user_acct=user * A + acct, account=acct, qos=rng.integers(0, Q, J), partition=np.zeros(J, np.uint32),
                      time_limit_sec=np.full(J, JOB_L, np.int64), select_index=sel, skip=skip)
    return _case(t, lj, dict(levels=acct, candidates=M, mask=cand), cores=cores)


def no_jobs() -> Case:
    """J = 0 limit jobs behind a cycle of three jobs"""
    c = sparse_candidates(3, "none")
    e = np.zeros(0, np.uint32)
    c.lj = lm.LimitJobs(user=e, user_acct=e, account=e, qos=e, partition=e, time_limit_sec=np.zeros(0, np.int64),
                        select_index=np.zeros(0, np.uint64), skip=np.zeros(0, np.uint8))
    c.info = dict(levels=e, candidates=0)
    return c


def input_usage(t: lm.LimitTables) -> lm.Usage:
    """the tables as cns_get_usage returns them when nothing was admitted"""
    u = t.empty_usage()
    for f in ("user_qos", "user_part", "acct_qos", "acct_part", "qos_usage"):
        if getattr(t, f) is not None:
            getattr(u, f)[:] = getattr(t, f)
        e = f + "_exists"
        if hasattr(u, e):
            getattr(u, e)[:] = 1 if getattr(t, e) is None else getattr(t, e)
    return u


def chain_of_seven() -> lm.LimitTables:
    """one account more than CNS_LIM_MAX_CHAIN in a row"""
    parent = [NONE] + list(range(lm.MAX_CHAIN))
    return lm.LimitTables(num_users=1, num_user_accts=len(parent), num_partitions=1, qos=np.array([lm.qos_limits()], lm.QOS_DT),
                          acct_parent=np.array(parent, np.uint32))


# ---- the cases of tests/test_gpu_limits_seams.py, by name: tests/test_limits_case.py proves their properties on the CPU ------------
HOT_KEYS = ("chunk-1", "chunk", "chunk+1", "2chunk+1", "row-1", "row", "row+1", "2row+1", "long_segment", "batch+1", "batch-1")
SEGMENT_KEYS = ("segment@chunk", "segment@row")
SCAN_KEYS = tuple("scan+300:" + p for p in PATTERNS[:4])
SMALL_KEYS = ("J=1", "J=255", "J=256", "J=257", "J=257:lane63")
EMPTY_KEYS = ("all_skipped", "J=0")
DEEP_KEYS = ("deep:1", "deep:2", "deep:3")
RECORD_KEYS = ("records:1", "records:2")
ALL_KEYS = HOT_KEYS + SEGMENT_KEYS + SCAN_KEYS + SMALL_KEYS + EMPTY_KEYS + DEEP_KEYS + RECORD_KEYS


def chunk_len(items: int, shp) -> int:
    """par_chunk_len of limits_kernels.hip from the shape's numbers"""
    c, nch = shp[0], shp[1]
    return max(c, -(-items // nch))


def seam_case(key: str, shp):
    """-> (generator name, arguments) for the shape cns_limits_shape reports"""
    c, nch, batch, rg, _, scan = shp
    row = rg * c                                       # items of one row group of the carry scan at the chunk floor
    deep = n_items([5])
    fewest = lambda L: -(-((L - 1) * nch + 1) // deep) * deep      # level-5 candidates: the fewest items whose chunk length is L
    hot_items = {"chunk-1": c - 1, "chunk": c, "chunk+1": c + 1, "2chunk+1": 2 * c + 1, "row-1": row - 1, "row": row, "row+1": row + 1,
                 "2row+1": 2 * row + 1, "long_segment": n_items([0]) * (2 * row + row // 2)}
    if key in hot_items:
        return "hot", (hot_items[key], 0)
    if key == "batch+1":                                # one item more than the floor: a batch of one item ends every chunk
        return "hot", (fewest(c + 1), 5)
    if key == "batch-1":                                # ... and a batch that misses one item
        return "hot", (fewest(next(L for L in range(c + 1, c + 2 * batch + 1) if L % batch == batch - 1)), 5)
    if key.startswith("segment@"):
        return "segment_on_last_item", (c if key == "segment@chunk" else row,)
    if key.startswith("scan+300:"):
        return "sparse_candidates", (scan + 300, key.split(":")[1])
    if key.startswith("J="):
        if key == "J=0":
            return "no_jobs", ()
        return "sparse_candidates", (int(key[2:].split(":")[0]), key.split(":")[1] if ":" in key else "stride_lastblock")
    if key == "all_skipped":
        return "sparse_candidates", (300, "none")
    if key.startswith("deep:"):
        return "deep_tree", (int(key[5:]),)
    if key.startswith("records:"):
        return "many_records", (int(key[8:]),)
    raise KeyError(key)


# ---- the rounds of the parallel pass as an algorithm, several records per job ---------------------------------------------------
def scalar_items(case: Case, placements, candidate):
    """The monotone checks of the candidates as (job, record, add, limit) items + usage0 per (record, component): every check of
    CheckRunLimits_ on a table WITHOUT GRES limits or requests and with every usage entry present is `usage + add <= limit` on
    one component (cpu, jobs, wall, mem) of one usage record.  candidate[J] bool: from the oracle (reason != 255)."""
    t, lj = case.t, case.lj
    Q, Pn, U, UA, A = t.num_qos, t.num_partitions, t.num_users, t.num_user_accts, t.num_accounts
    for f in ("user_qos_exists", "user_part_exists", "acct_qos_exists", "acct_part_exists"):
        assert getattr(t, f) is None or getattr(t, f).all(), "scalar_items: every usage entry must exist"
    assert not t.qos["max_tres"]["name_mask"].any() and not t.qos["max_tres_per_user"]["name_mask"].any() and \
        not t.qos["max_tres_per_account"]["name_mask"].any() and not (len(t.part_limits) and t.part_limits["max_tres"]["name_mask"].any())
    base = np.cumsum([0, U * Q, UA * Pn, A * Q, A * Pn])           # user_qos | user_part | acct_qos | acct_part | qos
    NR = int(base[-1]) + Q
    use0 = np.zeros((NR, 4), np.int64)
    for b, tab in zip(base, (t.user_qos, t.user_part, t.acct_qos, t.acct_part, t.qos_usage)):
        if tab is not None:
            use0[b:b + len(tab)] = np.stack([tab["cpu_raw"], tab["jobs_count"].astype(np.int64), tab["wall_sec"], tab["mem"].astype(np.int64)], 1)
    INF = np.iinfo(np.int64).max
    unl = lambda x: int(x["cpu_raw"]) == lm.UNLIMITED_CPU_RAW and int(x["mem"]) == lm.MAX_JOB_MEMORY
    wall_of = lambda w: int(w) if int(w) > 0 else INF
    job, rec, comp, add, lim = [], [], [], [], []
    ks = np.flatnonzero(candidate)
    sel = lj.select_index.astype(np.int64) if lj.select_index is not None else np.arange(lj.num_jobs)
    po = placements.place_offsets.astype(np.int64)
    for k, i in enumerate(ks):
        s = sel[i]
        rows = [r for r in range(po[s], po[s + 1]) if placements.node_idx[r] != abi.NODE_NONE]
        a4 = (sum(int(placements.cpu_raw[r]) for r in rows), 1, int(lj.time_limit_sec[i]), sum(int(placements.mem[r]) for r in rows))
        q = t.qos[lj.qos[i]]
        qi, p = int(lj.qos[i]), int(lj.partition[i])

        def put(r, limits):
            for c in range(4):
                if limits[c] != INF:
                    job.append(k); rec.append(r); comp.append(c); add.append(a4[c]); lim.append(limits[c])

        def part(r, pl_id, jobs_unl, tres_unl):
            if pl_id == NONE:
                return
            pl = t.part_limits[pl_id]
            tr = tres_unl
            put(r, (int(pl["max_tres"]["cpu_raw"]) if tr else INF, int(pl["max_jobs"]) if jobs_unl else INF,
                    wall_of(pl["max_wall_sec"]) if int(q["max_wall_sec"]) == 0 else INF, int(pl["max_tres"]["mem"]) if tr else INF))

        w = wall_of(q["max_wall_sec"])
        tpu, tpa, tg = q["max_tres_per_user"], q["max_tres_per_account"], q["max_tres"]
        put(int(base[0]) + int(lj.user[i]) * Q + qi, (min(int(q["max_cpus_per_user_raw"]), int(tpu["cpu_raw"])), int(q["max_jobs_per_user"]), w, int(tpu["mem"])))
        x = int(lj.user_acct[i])
        part(int(base[1]) + x * Pn + p, int(t.user_part_limit[x * Pn + p]) if t.user_part_limit is not None else NONE,
             int(q["max_jobs_per_user"]) == lm.UNLIMITED_JOBS, unl(tpu))
        a = int(lj.account[i])
        while a != NONE:
            put(int(base[2]) + a * Q + qi, (int(tpa["cpu_raw"]), int(q["max_jobs_per_account"]), w, int(tpa["mem"])))
            part(int(base[3]) + a * Pn + p, int(t.acct_part_limit[a * Pn + p]) if t.acct_part_limit is not None else NONE,
                 int(q["max_jobs_per_account"]) == lm.UNLIMITED_JOBS, unl(tpa))
            a = int(t.acct_parent[a])
        put(int(base[4]) + qi, (int(tg["cpu_raw"]), int(q["max_jobs"]), w, int(tg["mem"])))
    key = np.asarray(rec, np.int64) * 4 + np.asarray(comp, np.int64)
    return dict(n=len(ks), job=np.asarray(job, np.int64), key=key, add=np.asarray(add, np.int64), lim=np.asarray(lim, np.int64),
                use0=use0.reshape(-1)[key] if len(key) else np.zeros(0, np.int64))


def bracket_rounds(items, max_rounds=10 ** 6):
    """tests/test_device_logic_models.py::bracketing over items: state 0 undecided / 1 admitted / 2 rejected; per round the sums
    over the earlier admitted (L) and the earlier not-rejected (U) jobs of every key; passes every check under U -> admitted, fails
    one under L -> rejected.  -> (admitted[n] bool, rounds), rounds = None if max_rounds did not decide every job."""
    n, job, add, lim, use0 = items["n"], items["job"], items["add"], items["lim"], items["use0"]
    order = np.lexsort((job, items["key"]))              # by key, inside a key by job: the stable sort of the device
    job, add, lim, use0, key = job[order], add[order], lim[order], use0[order], items["key"][order]
    head = np.ones(len(key), bool)
    head[1:] = key[1:] != key[:-1]
    seg = np.cumsum(head) - 1
    first = np.flatnonzero(head)

    def excl(v):                                          # segmented exclusive prefix sum
        c = np.cumsum(v) - v
        return c - c[first][seg]

    state = np.zeros(n, np.uint8)
    rounds = 0
    while (state == 0).any():
        if rounds == max_rounds:
            return state == 1, None
        rounds += 1
        st = state[job]
        sL, sU = excl(np.where(st == 1, add, 0)), excl(np.where(st != 2, add, 0))
        not_pass = np.zeros(n, bool)
        fail = np.zeros(n, bool)
        not_pass[job[use0 + sU + add > lim]] = True
        fail[job[use0 + sL + add > lim]] = True
        und = state == 0
        new = state.copy()
        new[und & ~not_pass] = 1
        new[und & not_pass & fail] = 2
        assert (new != state).any(), "a round must decide at least the first undecided job"
        state = new
    return state == 1, rounds
