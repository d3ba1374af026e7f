"""Inputs for cns_schedule_steps at the edges that `tests.test_steps.random_step_case` (jobs of 1-6 nodes, node_num <= 4, tmax <= 4) and
`tests.gres_wide.step_case` (1-4 nodes, node_num <= 3) never reach (include/crane_gpu/steps.h, cranesched_amd/csrc/steps_kernels.hip).

Every family returns `(layout, StepJobs, Steps)`; `exact_fit` adds its hand-written expectations as a fourth value.  Five families:

  deep_heap        jobs of 1 .. 96 nodes around the heap's capacity (CNS_STEP_MAX_NODES = 64, one more entry while a node is evicted), steps of
                   1, 2, half, all but one and all of the job's nodes, few distinct task counts per node: the top-k queue holds up to 65
                   entries, most of them tied, and every sift path of libstdc++'s heap down to depth 6 runs;
  eviction_ladder  deterministic: 80 nodes whose task counts climb 1 .. 5 over and over, steps of 64 / 33 / 32 nodes that need the best
                   nodes of the WHOLE walk (every node behind the first node_num is pushed onto a full queue), and a job whose walk stops
                   on the very node that fills the queue;
  task_gres        deep_heap's shapes at a quarter of the node counts, every task request carrying GRES (untyped, typed, a second name),
                   some steps with a per-node GRES request in front of the tasks; on the three-class layout of the other step tests and on
                   one uneven wide layout of tests.gres_wide;
  exact_fit        hand-derived: availability taken to exactly zero and then one raw cpu unit / one byte more, tmin above what a node holds,
                   the spare tasks running out before the last node, include / exclude lists that name strangers, each other, everybody,
                   core ids on both sides of 64, 128 and 192 in one allocation;
  launch_shapes    0, 1, 63, 64, 65, 129 jobs (one thread per job in blocks of 64), jobs without steps, a job without nodes, no steps at all.

The sizes are the smallest that reach the edge.  tests/test_steps_edge.py asserts from ORACLE output that each family reaches what it is for,
before tests/test_gpu_steps_edge.py hands the same cases to the engine."""
from __future__ import annotations

import numpy as np

from cranesched_amd import steps as st
from tests import gres_wide, helpers
from tests.test_steps import GIB, _jobs, _steps

NODE_COUNTS = (1, 2, 31, 32, 33, 63, 64, 65, 80, 96)     # a job's allocation may be wider than CNS_STEP_MAX_NODES: only a step's node_num is capped
BLOCK = 64                                                # threads (= jobs) per workgroup of k_sched_steps
NOT_IN_JOB = 0xFFFFFFFE                                   # what the adapter puts into an include list for a node name it does not know
STEP_GRES_MASKS = (0, 0, 0x0F, 0xF3, 0xFF00, 0x3C5A)      # random_step_case's node slot masks


def _shapes(rng, J: int, scale: int, node_gres):
    """J jobs whose node counts cycle through NODE_COUNTS / scale, nodes with 1-8 free cores; per job 1-6 step specs (tests.test_steps._steps)."""
    job_nodes, nsteps, specs = [], [], []
    for j in range(J):
        n = max(1, -(-NODE_COUNTS[j % len(NODE_COUNTS)] // scale))
        nodes = sorted(rng.choice(500, n, replace=False).tolist())
        cores = rng.integers(1, 9, n)
        job_nodes.append([(nodes[i], int(cores[i]), 64, (1 << int(cores[i])) - 1, node_gres(rng)) for i in range(n)])
        nsteps.append(int(rng.integers(1, 7)))
        for _ in range(nsteps[-1]):
            k = int(np.clip(rng.choice([1, 2, n // 2, n - 1, n]), 1, min(n, st.STEP_MAX_NODES)))
            tmax = int(rng.integers(1, 7))
            d = dict(k=k, ntasks=int(rng.integers(k, k * tmax + 1)), tmin=min(tmax, int(rng.integers(1, 3))), tmax=tmax,
                     ncpu=int(rng.integers(0, 2)), cpu=float(rng.choice([0.5, 1, 2])))
            if rng.random() < 0.1:
                d["excl"] = rng.choice(nodes, min(n, int(rng.integers(1, 4))), replace=False).tolist()
            specs.append(d)
    return _jobs(job_nodes, nsteps), _steps(specs)


def deep_heap(seed: int, J: int = 24):
    rng = np.random.default_rng([seed, 7100])
    jobs, steps = _shapes(rng, J, 1, lambda r: 0)
    return helpers.multi_type_layout(), jobs, steps


LADDER_NODES = 80
LADDER_EARLY_NODES = 40


def eviction_ladder():
    # job 0: node i has (i % 5) + 1 cores and as many GiB: 16 nodes of each of 1 .. 5.
    #   step 0 (64 nodes, tasks of 1 cpu and no memory, <= 5 per node): the best 64 of all 80 hold 16 * (2 + 3 + 4 + 5) = 224 tasks, the best
    #     64 of the first 79 only 220 (the last node holds 5, a node of 1 takes its place): with ntasks = 224 the walk reaches the last node,
    #     every node from the 65th on is pushed onto a full queue, and the 16 one-core nodes are the ones that leave it.
    #   step 1 (33 nodes, tasks of 1 GiB and no cpu): the memory is untouched; the best 33 hold 16 * 5 + 16 * 4 + 3 = 147, the best 33 of the
    #     first 79 only 145: again the whole walk, evictions at queue size 34.
    #   step 2 (32 nodes, 1 GiB): what step 1 left is 15 nodes of 3 GiB, 16 of 2, 16 of 1: the best 32 hold 15 * 3 + 16 * 2 + 1 = 78.
    # job 1: 40 nodes of 2 cores; 32 nodes, 64 tasks, <= 2 per node: the 32nd node fills the queue AND brings the sum to 64: the walk stops
    #   there (CtldPublicDefs.cpp:2099-2101) and the step lists exactly the job's first 32 nodes.
    ladder = [(10 + 3 * i, (i % 5) + 1, (i % 5) + 1, (1 << ((i % 5) + 1)) - 1, 0) for i in range(LADDER_NODES)]
    early = [(300 + i, 2, 8, 0b11, 0) for i in range(LADDER_EARLY_NODES)]
    jobs = _jobs([ladder, early], [3, 1])
    steps = _steps([dict(k=64, ntasks=224, cpu=1, mem_gib=0, tmax=5), dict(k=33, ntasks=147, cpu=0, mem_gib=1, tmax=5),
                    dict(k=32, ntasks=78, cpu=0, mem_gib=1, tmax=5), dict(k=32, ntasks=64, cpu=1, mem_gib=0, tmax=2)])
    return helpers.multi_type_layout(), jobs, steps


def task_gres(seed: int, layout: str | None = None, J: int = 30):
    """layout None: the three-class layout of tests.helpers; else a name of tests.gres_wide.LAYOUTS."""
    rng = np.random.default_rng([seed, 7200, 0 if layout is None else 1])
    if layout is None:
        lay = helpers.multi_type_layout()
        masks = STEP_GRES_MASKS + (0xFFFF,)
    else:
        lay = gres_wide.make_layout(layout)
        masks = tuple(gres_wide._gres_kinds(lay, rng, 8))
    jobs, steps = _shapes(rng, J, 4, lambda r: int(masks[int(r.integers(0, len(masks)))]))
    S = steps.num_steps
    C, names = len(lay.class_name), sorted(set(lay.class_name))
    of_name = {a: [c for c in range(C) if lay.class_name[c] == a] for a in names}
    tgt, tgs = np.zeros((S, 4), np.uint8), np.zeros((S, 8), np.uint8)
    ngt, ngs = np.zeros((S, 4), np.uint8), np.zeros((S, 8), np.uint8)
    for s in range(S):
        sel = int(rng.integers(0, 3))
        if sel == 0:                                        # untyped, first name
            tgt[s, names[0]] = rng.integers(1, 3)
        elif sel == 1:                                      # typed
            c = int(rng.choice(of_name[names[0]])); v = int(rng.integers(1, 3))
            tgs[s, c] = v; tgt[s, names[0]] = v
        else:                                               # a second name
            tgt[s, names[1]] = rng.integers(1, 4)
        if rng.random() < 0.25:                             # the per-node request is taken first, the tasks see what is left
            if rng.random() < 0.5:
                ngt[s, names[int(rng.integers(0, 2))]] = 1
            else:
                c = int(rng.integers(0, C)); ngs[s, c] = 1; ngt[s, lay.class_name[c]] = 1
    steps.task_gres_total, steps.task_gres_spec, steps.node_gres_total, steps.node_gres_spec = tgt, tgs, ngt, ngs
    return lay, jobs, steps


def without_task_gres(steps: st.Steps, s: int) -> st.Steps:
    """A copy of `steps` whose step s asks for no GRES per task."""
    gt, gs = steps.task_gres_total.copy(), steps.task_gres_spec.copy()
    gt[s] = 0; gs[s] = 0
    return st.Steps(steps.node_cpu_raw, steps.node_mem, steps.task_cpu_raw, steps.task_mem, steps.node_num, steps.ntasks, steps.tmin, steps.tmax,
                    steps.node_gres_total, steps.node_gres_spec, gt, gs, steps.incl_offsets, steps.incl_nodes, steps.excl_offsets, steps.excl_nodes)


def exact_fit():
    """(layout, jobs, steps, exp).  exp: per step `scheduled`, and for the scheduled ones their node / task records in order (as
    tests.test_steps.scenario_fifo writes them, derived from CtldPublicDefs.cpp:2038-2159 and PublicHeader.cpp:519-599 before running
    anything); `avail_cpu` / `avail_mem` / `avail_core_lo` per (job, node) row."""
    jn, js, sp = [], [], []
    exp = dict(scheduled=[], node_idx=[], node_ntasks=[], task_node=[], task_core_lo=[], avail_cpu=[], avail_mem=[], avail_core_lo=[])

    def job(nodes, specs, scheduled, node_idx=(), node_ntasks=(), task_node=(), task_core_lo=(), avail_cpu=(), avail_mem=(), avail_core_lo=()):
        """node_idx .. task_core_lo: the records of the job's SCHEDULED steps, one after the other"""
        jn.append(nodes); js.append(len(specs)); sp.extend(specs)
        exp["scheduled"].append(list(scheduled))
        for key, v in (("node_idx", node_idx), ("node_ntasks", node_ntasks), ("task_node", task_node), ("task_core_lo", task_core_lo)):
            exp[key].append(list(v))
        exp["avail_cpu"] += list(avail_cpu); exp["avail_mem"] += list(avail_mem); exp["avail_core_lo"] += list(avail_core_lo)

    # job 0, cpu to exactly zero: n0 has 4 cores {0..3}, 8 GiB.  Two steps of 2 tasks x 1 cpu x 1 GiB take cores {0}, {1} and {2}, {3}:
    #   0 cpu, no core, 4 GiB left.  The third step asks for ONE raw unit (1/256 cpu): 1 > 0 (PublicHeader.cpp:522): pending.
    job([(0, 4, 8, 0xF, 0)],
        [dict(k=1, ntasks=2, cpu=1, tmax=2), dict(k=1, ntasks=2, cpu=1, tmax=2), dict(k=1, ntasks=1, cpu=1 / 256, mem_gib=0)],
        [1, 1, 0], node_idx=[0, 0], node_ntasks=[2, 2], task_node=[0, 0, 0, 0], task_core_lo=[0b0001, 0b0010, 0b0100, 0b1000],
        avail_cpu=[0], avail_mem=[4 * GIB], avail_core_lo=[0])
    # job 1, memory to exactly zero: n1 has 4 cores, 2 GiB.  2 tasks x half a cpu (no core id: PublicHeader.cpp:528-530) x 1 GiB: 3 cpus and
    #   0 bytes left.  The second step asks for ONE byte (task_mem is patched below): 1 > 0 (:523): pending.
    job([(1, 4, 2, 0xF, 0)],
        [dict(k=1, ntasks=2, cpu=0.5, tmax=2), dict(k=1, ntasks=1, cpu=0.5, mem_gib=0)],
        [1, 0], node_idx=[1], node_ntasks=[2], task_node=[1, 1], task_core_lo=[0, 0], avail_cpu=[3 * 256], avail_mem=[0], avail_core_lo=[0xF])
    one_byte_step = 4
    # job 2, tmin above what a node holds: n2 1 core, n3 and n4 3 cores; 2 nodes, 4 tasks, 2 .. 3 per node.  n2 holds 1 < 2: skipped (:2089-2091);
    #   n3 (3), n4 (3): 2 nodes, 6 >= 4 tasks.  Equal counts: the second push moves nothing, n3 is the top.  rest = 4 - 2 = 2: n3 gets
    #   min(2, 3-1) + 1 = 3 tasks, rest = 0, n4 gets 1.
    job([(2, 1, 8, 0b1, 0), (3, 3, 8, 0b111, 0), (4, 3, 8, 0b111, 0)], [dict(k=2, ntasks=4, cpu=1, tmin=2, tmax=3)],
        [1], node_idx=[3, 4], node_ntasks=[3, 1], task_node=[3, 3, 3, 4], task_core_lo=[0b001, 0b010, 0b100, 0b001],
        avail_cpu=[256, 0, 2 * 256], avail_mem=[8 * GIB, 5 * GIB, 7 * GIB], avail_core_lo=[0b1, 0, 0b110])
    # job 3, rest runs out before the last node: n5, n6, n7 with 2 cores each; 3 nodes, 4 tasks, <= 2 per node.  Three equal entries, no push
    #   moves anything: top n5 gets min(1, 1) + 1 = 2, rest = 0.  pop at size 3 (__adjust_heap on 2 entries: the lone left child moves up,
    #   the old last entry n7 goes below it): n6 is the top and gets 1 task, then n7 gets 1.
    job([(5, 2, 8, 0b11, 0), (6, 2, 8, 0b11, 0), (7, 2, 8, 0b11, 0)], [dict(k=3, ntasks=4, cpu=1, tmax=2)],
        [1], node_idx=[5, 6, 7], node_ntasks=[2, 1, 1], task_node=[5, 5, 6, 7], task_core_lo=[0b01, 0b10, 0b01, 0b01],
        avail_cpu=[0, 256, 256], avail_mem=[6 * GIB, 7 * GIB, 7 * GIB], avail_core_lo=[0, 0b10, 0b10])
    # job 4, include lists: n8, n9 with 2 cores.  Step 0 includes {n9, a node the job does not own}: only n9 qualifies.  Step 1 includes only
    #   the stranger: no node, pending.
    job([(8, 2, 8, 0b11, 0), (9, 2, 8, 0b11, 0)],
        [dict(k=1, ntasks=1, cpu=1, incl=[9, NOT_IN_JOB]), dict(k=1, ntasks=1, cpu=1, incl=[NOT_IN_JOB])],
        [1, 0], node_idx=[9], node_ntasks=[1], task_node=[9], task_core_lo=[0b01],
        avail_cpu=[2 * 256, 256], avail_mem=[8 * GIB, 7 * GIB], avail_core_lo=[0b11, 0b10])
    # job 5, a node in both lists: n10 is included and excluded: the exclusion is tested first (:2067-2072): n11.
    job([(10, 2, 8, 0b11, 0), (11, 2, 8, 0b11, 0)], [dict(k=1, ntasks=1, cpu=1, incl=[10, 11], excl=[10])],
        [1], node_idx=[11], node_ntasks=[1], task_node=[11], task_core_lo=[0b01],
        avail_cpu=[2 * 256, 256], avail_mem=[8 * GIB, 7 * GIB], avail_core_lo=[0b11, 0b10])
    # job 6, the exclude list covers the whole job: pending.
    job([(12, 2, 8, 0b11, 0), (13, 2, 8, 0b11, 0)], [dict(k=1, ntasks=1, cpu=1, excl=[13, 12])],
        [0], avail_cpu=[2 * 256, 2 * 256], avail_mem=[8 * GIB, 8 * GIB], avail_core_lo=[0b11, 0b11])
    # job 7, core ids on both sides of 64, 128 and 192: n14 has the 12 cores {62..65, 126..129, 190..193}; 4 tasks of 3 cpus take the lowest
    #   ids each (PublicHeader.cpp:533-538): {62, 63, 64}, {65, 126, 127}, {128, 129, 190}, {191, 192, 193}.
    straddle = sum(1 << i for i in (62, 63, 64, 65, 126, 127, 128, 129, 190, 191, 192, 193))
    job([(14, 12, 16, straddle, 0)], [dict(k=1, ntasks=4, cpu=3, tmax=4)],
        [1], node_idx=[14], node_ntasks=[4], task_node=[14] * 4, task_core_lo=[0b11 << 62, 0, 0, 0],
        avail_cpu=[0], avail_mem=[12 * GIB], avail_core_lo=[0])
    exp["straddle"] = dict(task_core_hi=[0b1, 0b10 | 0b11 << 62, 0, 0], task_core_w2=[0, 0, 0b11 | 1 << 62, 1 << 63], task_core_w3=[0, 0, 0, 0b11],
                           node_core=straddle)
    jobs, steps = _jobs(jn, js), _steps(sp)
    steps.task_mem[one_byte_step] = 1
    return helpers.multi_type_layout(), jobs, steps, exp


LAUNCH_SIZES = (0, 1, 63, 64, 65, 129)


def launch_shapes(J: int, no_steps: bool = False):
    """J jobs of 1-2 nodes and 0-2 steps.  The jobs on both sides of a block boundary (63 | 64, 127 | 128) own a step that fits whatever
    the seed says; job 5 (J > 5) owns NO node but one step, which stays pending.  no_steps: jobs, and not one step."""
    rng = np.random.default_rng([J, 7300])
    edge = {b * BLOCK - 1 for b in (1, 2)} | {b * BLOCK for b in (1, 2)}
    job_nodes, nsteps, specs = [], [], []
    for j in range(J):
        n = 0 if j == 5 else int(rng.integers(1, 3))
        job_nodes.append([(2 * j + i, 2, 4, 0b11, 0) for i in range(n)])
        ns = 0 if no_steps else 1 if j == 5 else int(rng.integers(1, 3)) if j in edge else int(rng.integers(0, 3))
        nsteps.append(ns)
        for i in range(ns):
            if j in edge and i == 0:
                specs.append(dict(k=1, ntasks=1, cpu=1))
            else:
                k = int(rng.integers(1, 3))
                specs.append(dict(k=k, ntasks=k + int(rng.integers(0, 3)), cpu=float(rng.choice([0.5, 1, 2])), tmax=2))
    return helpers.multi_type_layout(), _jobs(job_nodes, nsteps), _steps(specs)


# ---------------------------------------------------------------------------------------------------------------------------------
# the cases both test files run: id -> () -> (layout, jobs, steps)
# ---------------------------------------------------------------------------------------------------------------------------------
DEEP_HEAP_SEEDS = (3, 7, 29)     # chosen on the CPU: the oracle alone schedules steps of 32, 33, 63 and 64 nodes over them
TASK_GRES_SEEDS = (0, 1)
TASK_GRES_WIDE = ("uneven", 0)

CASES = {f"deep_heap-{s}": (lambda s=s: deep_heap(s)) for s in DEEP_HEAP_SEEDS}
CASES["eviction_ladder"] = eviction_ladder
CASES.update({f"task_gres-{s}": (lambda s=s: task_gres(s)) for s in TASK_GRES_SEEDS})
CASES[f"task_gres-{TASK_GRES_WIDE[0]}-{TASK_GRES_WIDE[1]}"] = lambda: task_gres(TASK_GRES_WIDE[1], layout=TASK_GRES_WIDE[0])
CASES["exact_fit"] = lambda: exact_fit()[:3]
CASES.update({f"launch-{J}": (lambda J=J: launch_shapes(J)) for J in LAUNCH_SIZES})
CASES["launch-no-steps"] = lambda: launch_shapes(3, no_steps=True)
