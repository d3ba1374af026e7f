"""The MultiFactorPriority sorter in front of a cycle, with the running side from the host and from the device ledger, at the shape
of profiles/r16_running_ledger.txt: 65 536 nodes in 8 partitions, 1 M running jobs (1.4 M allocations), 1 M pending jobs, 64 accounts,
per step 1 % of the seeded jobs retired and a queue of 10 000 one-node jobs scheduled by a real cycle and admitted.

Inside every step of one process, alternating:
  (a) cns_priority_order on a second handle with the seven running arrays handed in from the host (the path without the columns);
  (b) cns_running_advance_attrs + cns_priority_order_resident on the handle that holds the ledger;
and, on a third handle that makes the same calls without attributes, cns_running_advance: the extra cost of carrying the columns.
--preempt adds the front of a cycle with preemption (setup_ms of cns_running_preempt_get_timing): cns_running_select_preempt_attrs
against cns_running_select_preempt fed the downloaded columns; the pending jobs of partition 0 carry a QoS that may preempt.
One warm-up step, then the medians (and the spread) of --steps.  Host clock around each call; HIP-event times as the engine reports
them.  Asserts that (a) and (b) give equal orders and priority bits.  Prints one JSON line.

usage: python tools/prio_resident_bench.py [--steps 5] [--small] [--preempt]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cranesched_amd import abi  # noqa: E402
from cranesched_amd.engine import GpuNodeSelector  # noqa: E402
from cranesched_amd.priority import PriorityConfig, PrioRunning, synth_priority_case  # noqa: E402

GIB = 1 << 30
FULL = np.uint64(0xFFFFFFFFFFFFFFFF)
NOW = 1_700_000_000


def cluster(n, parts):
    nodes = np.arange(n, dtype=np.uint32)
    off = (np.arange(parts + 1) * (n // parts)).astype(np.uint32)
    return abi.Cluster(np.full(n, 128 * 256, np.int64), np.full(n, 512 * GIB, np.uint64), np.full(n, FULL), np.full(n, FULL), np.zeros(n, np.uint64), off, nodes)


def running_set(rng, n, R):
    """60 % of the jobs on one node, 40 % on two: 1.4 allocations per job; an allocation is one core's share without a core mask."""
    width = np.where(rng.random(R) < 0.6, 1, 2).astype(np.uint32)
    off = np.zeros(R + 1, np.uint32)
    off[1:] = np.cumsum(width)
    A = int(off[-1])
    owner = np.repeat(np.arange(R), width)
    node = ((owner * 7 + np.arange(A) - off[owner]) % n).astype(np.uint32)
    z = np.zeros(A, np.uint64)
    return abi.Running(end_sec=NOW + 3600 + (np.arange(R) % 1000), alloc_offsets=off, alloc_node=node, alloc_cpu_raw=np.full(A, 1, np.int64) + (owner % 4),
                       alloc_mem=(1 + owner % 3).astype(np.uint64), alloc_core_lo=z, alloc_core_hi=z, alloc_gres=z)


def queue(rng, q, parts):
    one = np.ones(q, np.uint32)
    return abi.Jobs(partition=rng.integers(0, parts, q).astype(np.uint32), time_limit_sec=np.full(q, 3600, np.int64), node_mem=np.zeros(q, np.uint64),
                    task_cpu_raw=np.full(q, 1, np.int64), task_mem=np.ones(q, np.uint64), node_num=one, ntasks=one, ntasks_per_node_min=one, ntasks_per_node_max=one)


def attrs(rng, n, accounts, start=None):
    return abi.RunningAttrs(qos=np.zeros(n), qos_priority=rng.choice([0, 10, 100, 1000], n), partition_priority=rng.choice([1, 5, 50], n), account=rng.integers(0, accounts, n),
                            start_sec=start)


def clock(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--small", action="store_true", help="100 000 running and pending jobs on 8 192 nodes")
    ap.add_argument("--preempt", action="store_true")
    a = ap.parse_args()
    n, R, J, Q, parts, accounts = (8192, 100_000, 100_000, 1000, 8, 64) if a.small else (65536, 1_000_000, 1_000_000, 10_000, 8, 64)
    rng = np.random.default_rng(18)
    c = cluster(n, parts)
    run = running_set(rng, n, R)
    ids = (1 + np.arange(R)).astype(np.uint32)
    seed_attrs = attrs(rng, R, accounts, start=NOW - rng.integers(1, 5 * 86400, R))
    pd = synth_priority_case(J, 0, accounts, 18, now=NOW)[0]
    cfg = PriorityConfig()
    eng, plain, host = GpuNodeSelector(device=0), GpuNodeSelector(device=0), GpuNodeSelector(device=0)
    eng.set_nodes(c)
    plain.set_nodes(c)
    _, t_seed_attrs = clock(lambda: eng.seed_running(run, ids, attrs=seed_attrs))
    _, t_seed = clock(lambda: plain.seed_running(run, ids))
    rows = {k: [] for k in ("host_order_ms", "resident_order_ms", "advance_attrs_ms", "advance_ms", "resident_kernels_ms", "host_kernels_ms", "advance_attrs_kernels_ms",
                            "advance_kernels_ms", "resident_second_call_ms", "preempt_attrs_setup_ms", "preempt_setup_ms")}
    next_id = 10_000_000
    for step in range(a.steps + 1):
        now = NOW + 60 * step
        jobs = queue(rng, Q, parts)
        eng.node_select(now, jobs)
        plain.node_select(now, jobs)
        retire = ids[step * (R // 100):(step + 1) * (R // 100)]
        job_ids = (next_id + np.arange(Q)).astype(np.uint32)
        next_id += Q
        qa = attrs(rng, Q, accounts)
        # (b) the boundary with the columns, then the sorter from the ledger
        got_adv, t_adv_attrs = clock(lambda: eng.advance_running(retire, now, job_ids, attrs=qa))
        k_adv_attrs = eng.running_timing()["kernels_ms"]
        want_adv, t_adv = clock(lambda: plain.advance_running(retire, now, job_ids))
        k_adv = plain.running_timing()["kernels_ms"]
        assert got_adv[1:] == want_adv[1:] and got_adv[2] > 0
        res, t_res = clock(lambda: eng.priority_order_resident(now + 30, cfg, accounts, pd))
        k_res = eng.priority_timing()["kernels_ms"]
        _, t_res2 = clock(lambda: eng.priority_order_resident(now + 30, cfg, accounts, pd))
        # (a) the same rows from the host (what a caller without the columns holds: not timed)
        at = eng.running_attrs()
        rn = PrioRunning(start_sec=at["start_sec"], qos_priority=at["qos_priority"], partition_priority=at["partition_priority"], node_num=at["node_num"],
                         alloc_cpu_raw=at["alloc_cpu_raw"], alloc_mem=at["alloc_mem"], account=at["account"])
        ref, t_host = clock(lambda: host.priority_order(now + 30, cfg, accounts, pd, running=rn))
        k_host = host.priority_timing()["kernels_ms"]
        assert res[2] == ref[2] and np.array_equal(res[0], ref[0]) and np.array_equal(res[1].view(np.uint64), ref[1].view(np.uint64)), "(a) and (b) differ"
        vals = {"host_order_ms": t_host, "resident_order_ms": t_res, "advance_attrs_ms": t_adv_attrs, "advance_ms": t_adv, "resident_kernels_ms": k_res, "host_kernels_ms": k_host,
                "advance_attrs_kernels_ms": k_adv_attrs, "advance_kernels_ms": k_adv, "resident_second_call_ms": t_res2}
        if a.preempt:
            led_ids = eng.running_ledger()[1]
            pq = (jobs.partition == 0).astype(np.uint32)
            args = ([[], [0]], job_ids, pq, np.full(Q, 20, np.uint32), Q - np.arange(Q, dtype=np.float64))
            fed = abi.Preempt(*args, led_ids, at["qos"], at["qos_priority"], at["start_sec"])
            bare = abi.Preempt(*args, [], [], [], [])
            x = eng.node_select_preempt_resident(now + 31, jobs, bare, from_attrs=True)
            vals["preempt_attrs_setup_ms"] = eng.preempt_setup_timing()["setup_ms"]
            y = plain.node_select_preempt_resident(now + 31, jobs, fed)
            vals["preempt_setup_ms"] = plain.preempt_setup_timing()["setup_ms"]
            assert x[0].diff(y[0]) is None and x[1].lists() == y[1].lists()
            admit = np.zeros(Q, np.uint8)   # (the cycle with preemption stands last on both handles: the next boundary is a plain retire)
            eng.advance_running([], now + 31, job_ids, admit, attrs=qa)
            plain.advance_running([], now + 31, job_ids, admit)
        if step:   # (step 0 is the warm-up)
            for k, v in vals.items():
                rows[k].append(v)
    out = {"shape": {"nodes": n, "running": R, "allocations": int(run.alloc_offsets[-1]), "pending": J, "accounts": accounts, "queue": Q, "retired_per_step": R // 100},
           "steps": a.steps, "seed_attrs_ms": round(t_seed_attrs, 3), "seed_ms": round(t_seed, 3), "orders_and_priority_bits_equal": True}
    for k, v in rows.items():
        if v:
            out[k] = {"median": round(float(np.median(v)), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
