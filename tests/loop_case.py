"""The controller loop of INTEGRATION.md 2 - 2l on ONE job universe, and its composed reference.

A universe is a list of job records; each carries everything every call needs of a job: id, user / user_acct / account / qos / partition,
submit time, held / begin time / dependencies (a tests/gate_pyref.Job), the row of its resource request in one abi.Jobs table, time
limit and reservation.  From the records the packers below (the existing ones: gate_case.pack, probe_case.take, usage_case.rows,
running_attrs_pyref.to_abi, the ABI classes' own constructors) build the inputs of every call.

scenario() runs the loop on the references alone, cycle after cycle, each step fed by what the step before left:

  a. gate_pyref.gate over the pending map                       -> the survivors, in ascending job id
  b. pyoracle.priority_order on AttrLedger.prio_running()       -> the order of the queue
  c. pyoracle.select on ledger.arrays() (with preemption: + abi.Preempt whose running side are the ledger's columns)
  d. commit_pyref.check on the cycle's placements               -> the codes
  e. pyoracle.run_limits with skip = code != COMMIT_OK          -> admitted, the tables
  f. AttrLedger.retire / admit                                  -> the ledger of the next cycle
  g. usage_pyref.apply(RELEASE) for the retired rows on the tables (e) left  -> the tables of the next cycle's (e)
  h. probe_case.expected against the cycle's final state

Between two cycles the universe moves: the admitted jobs leave the pending map, arrivals join it (their submit counts are charged on the
host, usage_pyref.apply(CHARGE)), dependency events fire for the rows that retired, pending jobs are cancelled, `now` advances.
tests/test_loop_case.py holds the scenario to its conditions without a GPU; tests/test_gpu_loop.py replays it on one engine handle."""
from __future__ import annotations

import copy
import ctypes as C
import dataclasses
from dataclasses import dataclass

import numpy as np

from cranesched_amd import abi, limits as lm, usage as us
from cranesched_amd.priority import PrioPending, PriorityConfig
from oracle import pyoracle
from tests import commit_pyref
from tests import gate_case
from tests import gate_pyref
from tests import helpers
from tests import probe_case as pc
from tests import running_attrs_pyref as rap
from tests import running_pyref as rp
from tests import usage_case as uc
from tests import usage_pyref as up

GIB = 1 << 30
NONE = lm.LIM_NONE
NODES, RUNNING, UNIVERSE, PROBES = 56, 30, 2600, 12
USERS, QOS, PARTS = 7, 3, 3
PARENT = [NONE, 0, 0, 1, NONE]            # accounts: a3 -> a1 -> a0, a2 -> a0, a4 a root
ACCOUNTS = len(PARENT)
ACCT_OF_USER = [1, 2, 3, 4, 3, 2, 4]      # one (user, account) pair per user: user_acct == user
LONE_USER = 6                             # submits nothing: its records hold its one running job alone, and are erased when it ends
QOS_PRIORITY = [10, 100, 1000]
PART_PRIORITY = [1, 5, 50]
QOS_PREEMPT = [[], [0], [1, 0]]           # QoS 2 may preempt 1 and 0, QoS 1 may preempt 0
CFG = PriorityConfig()
FAILED_DEPENDEE = 9                       # a job that failed: its event arrives at InfiniteFuture
NEVER_DEPENDEE = 7                        # a job nobody ever reports on
HANDOFFS = ("gate", "order", "codes", "admitted", "ledger", "tables")
STEPS = ("a", "b", "c", "d", "e", "f", "g", "h")


def shapes():
    """(job_chunk of the running ledger's kernels, job_chunk of the gate's): the workgroup seams the queue lengths must cross."""
    from cranesched_amd.engine import lib
    v = [C.c_uint32(0) for _ in range(4)]
    assert lib().cns_running_shape(*[C.byref(x) for x in v]) == 0
    g = [C.c_uint32(0) for _ in range(3)]
    assert lib().cns_gate_shape(*[C.byref(x) for x in g]) == 0
    return v[0].value, g[0].value


@dataclass
class JobRec:
    id: int
    row: int                      # the job's row in Universe.table: its abi.Jobs resource request, time limit and reservation
    user: int
    account: int
    qos: int
    partition: int
    submit: int
    time_limit: int
    reservation: int
    gate: gate_pyref.Job          # held / begin time / dependencies
    arrived: int = 0              # the cycle it joined the pending map in

    @property
    def user_acct(self):
        return self.user


@dataclass
class Cycle:
    """Every input and every expected output of one cycle.  Inputs that are packed from ids are kept as ids: the device test packs
    them from what the device answered, with the same packers."""
    now: int
    next_now: int
    arrivals: list                # the ids that joined the pending map in front of the cycle (a submit count each, charged on the host)
    # a
    pending_ids: list
    gate_jobs: abi.GateJobs
    gate_events: list
    gate: gate_pyref.Result
    dep_erased: np.ndarray
    survivors: list
    # b
    prio_pending: PrioPending
    order: np.ndarray
    priority: np.ndarray
    queue_ids: list
    # c
    jobs: abi.Jobs
    before: rap.AttrLedger
    oracle: object
    timelines: dict
    preempt: "abi.Preempt | None"
    preempting_in: list
    lists: list
    cancelled: list
    preempting_out: list
    # d
    commit_events: abi.CommitEvents
    gone: np.ndarray
    code: np.ndarray
    counts: np.ndarray
    # e
    tables_in: us.UsageState
    limit_reason: np.ndarray
    admitted: int
    usage: lm.Usage
    blind_reason: np.ndarray      # the same admission without the codes as skip
    # f
    retire: np.ndarray
    job_ids: np.ndarray
    admit: np.ndarray
    found: np.ndarray
    num_retired: int
    num_admitted: int
    after: rap.AttrLedger
    # g
    release_ids: list
    left_ids: list
    tables_before_release: us.UsageState
    not_found: np.ndarray
    over_free: np.ndarray
    tables_out: us.UsageState
    erased: int                   # nested records the release erased
    # h
    probe_rows: list
    probes: "abi.Jobs | None"
    probe_expected: "abi.Placements | None"
    held_all: bool = False


class Universe:
    """The cluster, the reservation table, the limits and every record; the packers of every call."""

    def __init__(self, seed: int):
        rng = np.random.default_rng(77000 + seed)
        c, table, now, run = helpers.random_case(seed, N=NODES, J=UNIVERSE, P=PARTS, running=RUNNING, lists=False)
        # three partitions, two of which share nodes 24 .. 39
        parts = [np.arange(0, 40), np.arange(24, 48), np.arange(48, NODES)]
        self.shared = set(range(24, 40))
        off = np.cumsum([0] + [len(p) for p in parts]).astype(np.uint32)
        self.cluster = abi.Cluster(c.cpu_total_raw, c.mem_total, c.core_lo, c.core_hi, c.gres_slots, off, np.concatenate(parts).astype(np.uint32),
                                   gres=c.gres, schedulable=c.schedulable)
        self.now0 = now
        self.layout = c.gres
        # one active reservation: a quarter of the cores of five nodes of partition 0, two of them shared with partition 1
        from tests.test_reservations import _resv
        al = []
        for n in (2, 5, 9, 26, 30):
            cores = int(c.cpu_total_raw[n] // 256)
            take = max(1, cores // 4)
            first = min(cores, 64) - take
            al.append((n, take, take, ((1 << take) - 1) << first))
        self.resv_allocs = al
        self.resv = _resv([(now - 300, now + 40000, al)])
        table.partition[:] = np.where(table.partition >= PARTS, rng.integers(0, PARTS, table.num_jobs), table.partition).astype(np.uint32)
        into = rng.random(table.num_jobs) < 0.12
        table.partition[into] = 0
        table.reservation = np.where(into, 0, abi.RESV_NONE).astype(np.uint32)
        table.skip = None
        self.table = table
        ptab = helpers.random_case(1000 + seed, N=NODES, J=60, P=PARTS, running=0, lists=False)[1]
        ptab.partition[:] = np.minimum(ptab.partition, PARTS + 1)      # (a partition that does not exist stays one)
        ptab.reservation = np.where(np.arange(60) % 5 == 0, 0, abi.RESV_NONE).astype(np.uint32)
        self.probe_table = ptab
        self.rng = rng
        self.recs: dict = {}
        self.next_row = 0
        self.next_id = 2000
        # the first running set: tests.helpers' rows, two rows inside the reservation, ids 1000 ..
        led = rp.Ledger.from_running(run, 1000 + np.arange(len(run.end_sec)))
        for k, (n, take, _, mask) in enumerate(al[:2]):
            led.rows.append(rp.Row(1000 + len(led.rows), now + 700 + 900 * k, 0,
                                   [(n, {"cpu_raw": 256, "mem": GIB // 2, "core_lo": mask & -mask, "core_hi": 0, "core_w2": 0, "core_w3": 0, "gres": 0})]))
        R = len(led.rows)
        attrs = rap.random_attrs(rng, R, ACCOUNTS, now)
        attrs["start_sec"] = [int(now - 1 - 7 * x) for x in rng.permutation(R)]        # all different (TryPreempt_'s comparator)
        attrs["qos"] = [int(x) for x in rng.integers(0, QOS, R)]
        attrs["qos_priority"] = [QOS_PRIORITY[q] for q in attrs["qos"]]
        users = [int(u) for u in rng.integers(0, LONE_USER, R)]
        users[int(np.argmin([r.end_sec for r in led.rows]))] = LONE_USER
        attrs["account"] = [ACCT_OF_USER[u] for u in users]
        self.first = rap.AttrLedger(led, attrs)
        # who the running jobs belong to (the release needs it)
        self.owner = {}
        for r, user, q in zip(led.rows, users, attrs["qos"]):
            part = 0 if r.reservation == 0 else int(rng.integers(0, PARTS))
            self.owner[r.job_id] = dict(user=user, account=ACCT_OF_USER[user], qos=q, part=part, wall=int(rng.integers(1, 100)) * 60)
        self.qos_limits = np.array([lm.qos_limits(max_jobs_per_user=8),
                                    lm.qos_limits(max_jobs_per_account=20, max_tres_per_account=lm.tres(cpu=160)),
                                    lm.qos_limits(max_jobs=30, max_cpus_per_user=64)], lm.QOS_DT)
        self.meta = us.UsageTables(layout=self.layout, num_users=USERS, num_user_accts=USERS, num_qos=QOS, num_partitions=PARTS, acct_parent=PARENT)

    # ---- the accounting tables ----------------------------------------------------------------------------------------------------
    def first_tables(self) -> us.UsageState:
        """Every entity exists and no record does; the running jobs are charged as a recovery charges them (:155-178)."""
        t = dataclasses.replace(self.meta, user_exists=np.ones(USERS, np.uint8), acct_exists=np.ones(ACCOUNTS, np.uint8), qos_exists=np.ones(QOS, np.uint8))
        rows = [self.release_row(r, self.owner[r.job_id]) for r in self.first.ledger.rows]
        return up.apply(self.meta, t.state(), abi.USAGE_CHARGE, uc.rows(*rows))[0]

    def alloc_counts(self, row: rp.Row):
        """cpu, mem, per-name totals and per-class counts of a ledger row's allocations (ResourceView += DedicatedResourceInNode)."""
        L = self.layout
        classes = [sum(bin((a[1]["gres"] >> int(L.class_shift[g])) & ((1 << int(L.class_width[g])) - 1)).count("1") for a in row.allocs) for g in range(len(L.class_name))]
        names = [0] * abi.MAX_GRES_NAMES
        for g, n in enumerate(classes):
            names[int(L.class_name[g])] += n
        return sum(a[1]["cpu_raw"] for a in row.allocs), sum(a[1]["mem"] for a in row.allocs), names, classes

    def release_row(self, row: rp.Row, who: dict) -> dict:
        """FreeMetaResource(JobInCtld) (:243-254) of a job that ended: its allocation, one job, one submit, its time limit."""
        cpu, mem, names, classes = self.alloc_counts(row)
        return dict(user=who["user"], account=who["account"], qos=who["qos"], part=who["part"], cpu=cpu, mem=mem, wall=who["wall"], jobs=1, submit=1,
                    names=names, classes=classes)

    def who(self, job_id: int) -> dict:
        if job_id in self.owner:
            return self.owner[job_id]
        r = self.recs[job_id]
        return dict(user=r.user, account=r.account, qos=r.qos, part=r.partition, wall=r.time_limit)

    def release_rows(self, ledger: rp.Ledger, ids, left=()) -> us.UsageJobs:
        """ids: ledger rows that ended; left: pending jobs that left the queue before they ran (FreeMetaSubmitResource, :226-241)."""
        by_id = {r.job_id: r for r in ledger.rows}
        return uc.rows(*[self.release_row(by_id[i], self.who(i)) for i in ids],
                       *[dict(user=self.recs[i].user, account=self.recs[i].account, qos=self.recs[i].qos, part=self.recs[i].partition, submit=1) for i in left])

    def submit_rows(self, ids) -> us.UsageJobs:
        """MallocMetaSubmitResource (:139-153): one submit per arrival."""
        return uc.rows(*[dict(user=self.recs[i].user, account=self.recs[i].account, qos=self.recs[i].qos, part=self.recs[i].partition, submit=1) for i in ids])

    def limit_tables(self, s: us.UsageState) -> lm.LimitTables:
        return lm.LimitTables(num_users=USERS, num_user_accts=USERS, num_partitions=PARTS, qos=self.qos_limits, acct_parent=np.array(PARENT, np.uint32),
                              user_qos=s.user_qos.copy(), user_qos_exists=s.user_qos_exists.copy(), user_part=s.user_part.copy(),
                              user_part_exists=s.user_part_exists.copy(), acct_qos=s.acct_qos.copy(), acct_qos_exists=s.acct_qos_exists.copy(),
                              acct_part=s.acct_part.copy(), acct_part_exists=s.acct_part_exists.copy(), qos_usage=s.qos_usage.copy())

    def with_usage(self, s: us.UsageState, u: lm.Usage) -> us.UsageState:
        """The tables after an admission: the nine arrays it writes replace the state's, the submit counts and entity bytes stay."""
        return dataclasses.replace(s, **{f: getattr(u, f).copy() for f in u.__dataclass_fields__})

    def usage_tables(self, s: us.UsageState) -> us.UsageTables:
        return dataclasses.replace(self.meta, **{f: getattr(s, f).copy() for f in s.__dataclass_fields__})

    # ---- the packers of the queue's calls -------------------------------------------------------------------------------------------
    def gate_jobs(self, ids) -> abi.GateJobs:
        return gate_case.pack([self.recs[i].gate for i in ids])

    def prio_pending(self, ids) -> PrioPending:
        r = [self.recs[i] for i in ids]
        rows = np.array([x.row for x in r], np.int64)
        t = self.table
        nt = t.ntasks[rows].astype(np.int64)
        return PrioPending(submit_sec=[x.submit for x in r], qos_priority=[QOS_PRIORITY[x.qos] for x in r], partition_priority=[PART_PRIORITY[x.partition] for x in r],
                           node_num=t.node_num[rows], total_cpu_raw=t.task_cpu_raw[rows] * nt, total_mem=t.task_mem[rows] * nt.astype(np.uint64),
                           account=[x.account for x in r])

    def jobs(self, ids) -> abi.Jobs:
        return pc.take(self.table, [self.recs[i].row for i in ids])

    def commit_jobs(self, jobs: abi.Jobs, gone, preempt_out=None, num_running=0) -> abi.CommitJobs:
        kw = {}
        if preempt_out is not None:    # every victim is still in the running map when the commit loop looks (:1546)
            kw = dict(preempt_offsets=preempt_out.offsets[:jobs.num_jobs + 1].copy(), preempted=preempt_out.preempted[:int(preempt_out.offsets[jobs.num_jobs])].copy(),
                      running_alive=np.ones(num_running, np.uint8))
        return abi.CommitJobs(time_limit_sec=jobs.time_limit_sec, reservation=jobs.reservation, gone=gone, **kw)

    def limit_jobs(self, ids, jobs: abi.Jobs, skip) -> lm.LimitJobs:
        r = [self.recs[i] for i in ids]
        return lm.LimitJobs(user=[x.user for x in r], user_acct=[x.user_acct for x in r], account=[x.account for x in r], qos=[x.qos for x in r],
                            partition=[x.partition for x in r], time_limit_sec=jobs.time_limit_sec, skip=skip)

    def queue_attrs(self, ids) -> dict:
        r = [self.recs[i] for i in ids]
        return {"qos": [x.qos for x in r], "qos_priority": [QOS_PRIORITY[x.qos] for x in r], "partition_priority": [PART_PRIORITY[x.partition] for x in r],
                "account": [x.account for x in r]}

    def preempt(self, ids, priority, ledger: "rap.AttrLedger | None", preempting) -> abi.Preempt:
        """ledger None: the running side stays empty (the device reads it from the columns)."""
        r = [self.recs[i] for i in ids]
        rn = ([], [], [], [])
        if ledger is not None:
            c = ledger.columns()
            rn = (ledger.ledger.ids(), c["qos"], c["qos_priority"], c["start_sec"])
        return abi.Preempt(QOS_PREEMPT, ids, [x.qos for x in r], [QOS_PRIORITY[x.qos] for x in r], priority, *rn, preempting=list(preempting))

    def probes(self, rows) -> abi.Jobs:
        return pc.take(self.probe_table, rows)

    # ---- arrivals -------------------------------------------------------------------------------------------------------------------
    def arrive(self, n: int, now: int, cycle: int, running_ids) -> list:
        rng, ids = self.rng, []
        for _ in range(n):
            row, self.next_row = self.next_row, self.next_row + 1
            assert row < self.table.num_jobs, "the universe's job table is used up"
            self.next_id += int(rng.integers(1, 4))                       # gaps between the ids
            g = gate_pyref.Job(self.next_id)
            u = rng.random()
            if u < 0.06:
                g.held = True
            elif u < 0.12:
                g.begin_time = now + int(rng.choice([1, 700, 1300]))
            elif u < 0.22 and len(running_ids):
                g.dependencies = gate_case.deps({int(rng.choice(running_ids)): int(rng.choice([0, 0, 5]))})
            elif u < 0.25 and len(running_ids) > 1:
                a, b = rng.choice(running_ids, 2, replace=False)
                g.dependencies = gate_case.deps({int(a): 0, int(b): 0}, True, gate_pyref.INF)
            elif u < 0.28:
                g.dependencies = gate_case.deps({FAILED_DEPENDEE: 0})
            elif u < 0.30:
                g.dependencies = gate_case.deps({NEVER_DEPENDEE: 0})
            user = int(rng.integers(0, LONE_USER))
            self.recs[self.next_id] = JobRec(self.next_id, row, user, ACCT_OF_USER[user], int(rng.integers(0, QOS)), int(self.table.partition[row]),
                                             now - int(rng.integers(0, 3 * 86400)), int(self.table.time_limit_sec[row]), int(self.table.reservation[row]), g, cycle)
            ids.append(self.next_id)
        return ids


# targets of the pending map's length per cycle, in units of the workgroup's job_chunk; (steps to the next now); what is special
PLAN = [dict(size=1.1, step=600), dict(size=1.9, step=600), dict(size=0.45, step=600), dict(size=0.7, step=600, hold_all=True),
        dict(size=1.5, step=1), dict(size=0.6, step=600)]


def draw_commit_events(rng, jobs: abi.Jobs, pl: abi.Placements, resv: abi.Reservations, cycle: int):
    """Node events on nodes that started jobs use, a second before, at and a second behind their ends; in the odd cycles the reservation
    ends inside its jobs' ends; 3 % of the jobs left the pending map since the cycle began."""
    J = jobs.num_jobs
    started = [int(j) for j in np.flatnonzero(pl.reason[:J] == 0)]
    end = pl.start_sec[:J] + jobs.time_limit_sec
    rec = lambda j: [int(n) for n in pl.node_idx[int(pl.place_offsets[j]):int(pl.place_offsets[j + 1])] if n != abi.NODE_NONE]
    plain = [j for j in started if jobs.reservation[j] == abi.RESV_NONE]
    node_events = []
    for j in (rng.choice(plain, min(len(plain), 5), replace=False).tolist() if plain else []):
        node_events.append((int(end[j]) + int(rng.choice([-1, -1, 0, 1])), [int(rng.choice(rec(j)))]))
    affected = []
    mine = sorted(int(end[j]) for j in started if jobs.reservation[j] == 0)
    if cycle % 2 == 1 and mine:
        lo, hi = int(resv.alloc_offsets[0]), int(resv.alloc_offsets[1])
        affected.append((0, 1, mine[-1] - 1, [int(n) for n in resv.alloc_node[lo:hi]]))      # a second short of its last job's end
    gone = (rng.random(J) < 0.03).astype(np.uint8)
    return abi.CommitEvents(node_events=node_events, affected_resv=affected), gone


def scenario(seed: int, preempt: bool = False, drop: "str | None" = None, chunk: "int | None" = None):
    """-> (universe, reservation table, first AttrLedger, first accounting tables, [Cycle]).  drop: one of HANDOFFS — the composed
    reference with that hand-off lost (tests/test_loop_case.py: a later expected output must change)."""
    assert drop is None or drop in HANDOFFS
    chunk = chunk or max(shapes())
    U = Universe(seed)
    rng = U.rng
    led = U.first.copy()
    state = U.first_tables()
    first_state = copy.deepcopy(state)
    pending: list = []
    events: list = []
    preempting: list = []
    now = U.now0
    out = []
    for c, plan in enumerate(PLAN):
        next_now = now + plan["step"]
        # ---- the universe moves: holds and begin times pass, users cancel, jobs arrive ------------------------------------------
        for i in pending:
            if U.recs[i].gate.held and U.recs[i].arrived < c - 1:
                U.recs[i].gate.held = False
        target = int(plan["size"] * chunk)
        if len(pending) > target:
            pending = pending[len(pending) - target:]                  # the oldest are cancelled
        new = U.arrive(target - len(pending), now, c, led.ledger.ids())
        if new:
            state = up.apply(U.meta, state, abi.USAGE_CHARGE, U.submit_rows(new))[0]
        pending = sorted(pending + new)
        events += [(i, FAILED_DEPENDEE, gate_pyref.INF) for i in pending if FAILED_DEPENDEE in U.recs[i].gate.dependencies.deps and U.recs[i].arrived < c]
        events.append((1, 2, now))                                     # an event for nobody
        held = []
        if plan.get("hold_all"):
            held = [i for i in pending if not U.recs[i].gate.held]
            for i in held:
                U.recs[i].gate.held = True
        # ---- a. the gate -----------------------------------------------------------------------------------------------------------
        gjobs = [U.recs[i].gate for i in pending]
        gate_in = U.gate_jobs(pending)
        res, erased, after = gate_case.expected(now, gjobs, events)
        for i, g in zip(pending, after):
            U.recs[i].gate = g
        survivors = [pending[r] for r in res.pending] if drop != "gate" else list(pending)
        # ---- b. the order ----------------------------------------------------------------------------------------------------------
        rows_b = (U.first if drop == "ledger" else led)
        pd = U.prio_pending(survivors)
        order, prio = pyoracle.priority_order(now, CFG, ACCOUNTS, pd, running=rows_b.prio_running() if rows_b.rows else None)
        order, prio = order.copy(), prio.copy()
        queue = [survivors[i] for i in (order if drop != "order" else range(len(survivors)))]
        # ---- c. the cycle ------------------------------------------------------------------------------------------------------------
        jobs = U.jobs(queue)
        J = jobs.num_jobs
        before = rows_b.copy()
        run, ids = before.ledger.arrays()
        run = run if len(ids) else None
        pre = U.preempt(queue, prio[order] if drop != "order" else prio, before, preempting) if preempt else None
        ora = pyoracle.select(U.cluster, jobs, now, running=run, reservations=U.resv, preempt=pre)
        pl = ora.placements
        touched = [n for n in _touched(before.ledger, pl)][:40]
        timelines = {n: ora.timeline(n) for n in touched}
        lists = ora.preempt_out.lists() if preempt else [[] for _ in range(J)]
        cancelled = ora.preempt_out.cancelled_ids() if preempt else []
        preempting_out = ora.preempt_out.preempting_ids() if preempt else []
        # ---- d. the commit loop's checks ---------------------------------------------------------------------------------------------
        cev, gone = draw_commit_events(rng, jobs, pl, U.resv, c)
        cj = U.commit_jobs(jobs, gone, ora.preempt_out if preempt else None, len(ids))
        code, counts = commit_pyref.check(pl.start_sec, pl.reason, pl.place_offsets, pl.node_idx, cev, cj)
        # ---- e. the run limits -------------------------------------------------------------------------------------------------------
        tables_in = copy.deepcopy(state)
        lt = U.limit_tables(tables_in)
        skip = (code != abi.COMMIT_OK).astype(np.uint8)
        blind, _, _ = pyoracle.run_limits(U.layout, lt, U.limit_jobs(queue, jobs, None), pl)
        lreason, adm, usage = pyoracle.run_limits(U.layout, lt, U.limit_jobs(queue, jobs, skip if drop != "codes" else None), pl)
        lreason, blind = lreason.copy(), blind.copy()
        state = U.with_usage(tables_in, usage)
        # ---- f. the boundary ---------------------------------------------------------------------------------------------------------
        retire = [r.job_id for r in led.ledger.rows if r.end_sec <= next_now]
        if plan["step"] > 1:                                           # (behind the short step nothing has ended and no cancel went through yet)
            retire += [x for x in cancelled if x not in retire] + [77]
        retire = np.array(retire, np.uint32)
        job_ids = np.array(queue, np.uint32)
        admit = (lreason == 0).astype(np.uint8) if drop != "admitted" else np.ones(J, np.uint8)
        ended = {r.job_id: r for r in led.ledger.rows}
        ledger_before = led.ledger.copy()
        found, nret = led.retire(retire)
        nadm = led.admit(pl, jobs.time_limit_sec, now, job_ids, U.queue_attrs(queue), admit, jobs.reservation) if J else 0
        # ---- g. the releases ---------------------------------------------------------------------------------------------------------
        release_ids = [int(i) for i, f in zip(retire, found) if f]
        left_ids = [queue[j] for j in range(J) if gone[j]] + [pending[r] for r in range(len(pending)) if res.code[r] == gate_pyref.DEPENDENCY_NEVER]
        tables_before = copy.deepcopy(state)
        nf = of = np.zeros(0, np.uint16)
        n_erased, tables_out = 0, copy.deepcopy(state)
        if release_ids or left_ids:
            released, nf, of = up.apply(U.meta, state, abi.USAGE_RELEASE, U.release_rows(ledger_before, release_ids, left_ids))
            n_erased = sum(int(((getattr(tables_before, e) != 0) & (getattr(released, e) == 0)).sum()) for e in lm.NESTED)
            tables_out = copy.deepcopy(released)
            if drop != "tables":
                state = released
        # ---- h. the probes -----------------------------------------------------------------------------------------------------------
        probe_rows, probes, pexp = [], None, None
        if not preempt:                                                # (cns_probe is not served behind a cycle with preemption)
            probe_rows = [int(x) for x in rng.choice(U.probe_table.num_jobs, PROBES, replace=False)]
            probes = U.probes(probe_rows)
            pexp = pc.expected(U.cluster, jobs, probes, now, running=run, reservations=U.resv)
        out.append(Cycle(now, next_now, list(new), list(pending), gate_in, list(events), res, erased, list(survivors), pd, order, prio, list(queue), jobs, before, ora,
                         timelines, pre, list(preempting), lists, cancelled, preempting_out, cev, gone, code, counts, tables_in, lreason, int(adm), usage, blind,
                         retire, job_ids, admit, found, nret, nadm, led.copy(), release_ids, left_ids, tables_before, nf, of, tables_out, n_erased,
                         probe_rows, probes, pexp, bool(plan.get("hold_all"))))
        # ---- the universe moves on ---------------------------------------------------------------------------------------------------
        for i in held:
            U.recs[i].gate.held = False
        left = {queue[j] for j in range(J) if admit[j] and int(pl.reason[j]) == 0 and int(pl.start_sec[j]) == now} | set(left_ids)
        pending = [i for i in pending if i not in left]
        events = [(i, int(d), ended[int(d)].end_sec) for d, f in zip(retire, found) if f for i in pending if int(d) in U.recs[i].gate.dependencies.deps]
        preempting = preempting_out
        now = next_now
    return U, U.resv, U.first, first_state, out


def _touched(ledger: rp.Ledger, pl: abi.Placements):
    s = {n for r in ledger.rows for n, _ in r.allocs}
    used = pl.node_idx[:pl.capacity]
    s.update(int(n) for n in used[used != abi.NODE_NONE])
    return sorted(s)


def cycle_key(c: Cycle):
    """The expected outputs of a cycle as bytes, step by step: two scenarios that differ in a hand-off differ in a key behind it."""
    J = c.jobs.num_jobs
    pl = c.oracle.placements
    t = c.tables_out
    return {"a": c.gate.code.tobytes() + c.gate.pending.tobytes(), "b": c.order.tobytes() + c.priority.tobytes(),
            "c": pl.start_sec[:J].tobytes() + pl.reason[:J].tobytes() + pl.node_idx[:int(pl.place_offsets[J])].tobytes() + repr((c.lists, c.cancelled)).encode(),
            "d": c.code.tobytes(), "e": c.limit_reason.tobytes() + b"".join(getattr(c.usage, f).tobytes() for f in c.usage.__dataclass_fields__),
            "f": repr(c.after.ledger.ids()).encode() + c.found.tobytes(), "g": b"".join(getattr(t, f).tobytes() for f in t.__dataclass_fields__),
            "h": b"" if c.probe_expected is None else c.probe_expected.start_sec.tobytes() + c.probe_expected.reason.tobytes()}
