"""Python restatement of the node walk of JobScheduler::CreateResv_ (src/CraneCtld/JobScheduler.cpp:4383-4419), the truth for
include/crane_gpu_resv/resv_probe.h.  Plain Python integers and loops, per node the lists the reference walks
(CranedMeta::rn_job_res_map -> the running jobs' end times, CranedMeta::resv_in_node_map -> (start, end) per reservation).

  at_start()   the loop as the reference has it — running first, then reservations, then "first k in order" — extended to code
               EVERY candidate (the reference breaks at the k-th free node, :4416-4418);
  earliest()   brute force: every time at which the free count can rise (the start, a candidate's running ends, the end of a
               reservation on a candidate), ascending, through at_start(); the first that succeeds.  On purpose not the sweep the
               device uses.
"""
from __future__ import annotations

import numpy as np

INT64_MAX = (1 << 63) - 1
OK, NOT_ENOUGH, IN_THE_PAST = 0, 1, 2
FREE, RUNNING, RESERVED, NOT_FOUND = 0, 1, 2, 3


class NodeState:
    """Per node: the end times of the running jobs on it and the (start, end) of the reservations that list it."""

    def __init__(self, num_nodes: int, running=None, reservations=None):
        self.num_nodes = num_nodes
        self.job_ends = [[] for _ in range(num_nodes)]
        self.resv = [[] for _ in range(num_nodes)]
        if running is not None:      # abi.Running: every allocation counts, whichever reservation the job runs in
            for j in range(len(running.end_sec)):
                for a in range(int(running.alloc_offsets[j]), int(running.alloc_offsets[j + 1])):
                    self.job_ends[int(running.alloc_node[a])].append(int(running.end_sec[j]))
        if reservations is not None:  # abi.Reservations: expired ones too (:4405 tests overlap only)
            for v in range(len(reservations.start_sec)):
                for a in range(int(reservations.alloc_offsets[v]), int(reservations.alloc_offsets[v + 1])):
                    self.resv[int(reservations.alloc_node[a])].append((int(reservations.start_sec[v]), int(reservations.end_sec[v])))


def at_start(state: NodeState, start: int, duration: int, k: int, cand):
    """-> (ok, num_free, codes, chosen) at `start`; end = start + duration saturates at INT64_MAX."""
    end = min(start + duration, INT64_MAX)           # :4320
    codes, free = [], []
    for n in cand:                                   # :4383
        if n >= state.num_nodes:                     # :4385-4388 nodes_not_found
            codes.append(NOT_FOUND)
            continue
        failed = False
        for job_end in state.job_ends[n]:            # :4391-4400
            if job_end > start:                      # :4395
                codes.append(RUNNING)
                failed = True
                break
        if failed:
            continue                                 # :4401
        for st, ed in state.resv[n]:                 # :4403-4410
            if st < end and ed > start:              # :4405
                codes.append(RESERVED)
                failed = True
                break
        if failed:
            continue                                 # :4411
        codes.append(FREE)
        free.append(n)                               # :4415 (the reference stops at the k-th, :4416-4418)
    ok = len(free) >= k                              # :4421
    return ok, len(free), codes, (free[:k] if ok else [])


def rise_times(state: NodeState, start: int, cand):
    """The times >= start at which the free count of `cand` can rise; INT64_MAX is an infinite end and is never reached."""
    ts = {start}
    for n in cand:
        if n >= state.num_nodes:
            continue
        ts.update(state.job_ends[n])
        ts.update(ed for _, ed in state.resv[n])
    return sorted(t for t in ts if start <= t < INT64_MAX)


def earliest(state: NodeState, start: int, duration: int, k: int, cand):
    """-> (t or None, ok, num_free, codes, chosen): the first rise time at which at_start succeeds, else the answer at `start`."""
    for t in rise_times(state, start, cand):
        ok, nf, codes, chosen = at_start(state, t, duration, k, cand)
        if ok:
            return t, ok, nf, codes, chosen
    ok, nf, codes, chosen = at_start(state, start, duration, k, cand)
    return None, ok, nf, codes, chosen


def answer(state: NodeState, now: int, queries) -> dict:
    """cns_resvq_run over abi.ResvQueries -> the arrays of cns_resvq_out."""
    Q = queries.num_queries
    status, start_out, num_free = np.zeros(Q, np.uint8), np.zeros(Q, np.int64), np.zeros(Q, np.uint32)
    code, chosen, choff = [], [], [0]
    for q in range(Q):
        b, e = int(queries.cand_offsets[q]), int(queries.cand_offsets[q + 1])
        cand = [int(x) for x in queries.cand_nodes[b:e]]
        start, dur = int(queries.start_sec[q]), int(queries.duration_sec[q])
        k = int(queries.node_num[q]) or len(cand)    # :4357-4358
        if start + dur <= now:                       # :4323
            status[q] = IN_THE_PAST
            code += [0] * len(cand)
            choff.append(len(chosen))
            continue
        if queries.find_earliest is not None and queries.find_earliest[q]:
            t, ok, nf, codes, ch = earliest(state, start, dur, k, cand)
        else:
            ok, nf, codes, ch = at_start(state, start, dur, k, cand)
            t = start
        status[q] = OK if ok else NOT_ENOUGH
        start_out[q] = t if ok else 0
        num_free[q] = nf
        code += codes
        chosen += ch
        choff.append(len(chosen))
    return {"status": status, "start_sec": start_out, "num_free": num_free, "code": np.array(code, np.uint8),
            "chosen_offsets": np.array(choff, np.uint64), "chosen_nodes": np.array(chosen, np.uint32)}
