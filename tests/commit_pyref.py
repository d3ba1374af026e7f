"""The commit loop's checks between NodeSelect and the admission (src/CraneCtld/JobScheduler.cpp:1464-1555), restated statement by
statement with the reference's line beside each: the truth for include/crane_gpu_commit/commit_check.h.  The block sits inside
ScheduleThread_ on the Ctld singletons and cannot be sliced into a library, so — as for CreateResv_ (tests/resvq_pyref.py) — it is
restated here and held to a hand-derived table (tests/test_commit_pyref.py).

It takes the placements as INPUT (start, reason, place offsets, node indices of a cycle: the oracle's or the engine's own download), the
events and job arrays of the call (abi.CommitEvents, abi.CommitJobs), and keeps the reference's oddities: no `break` in the
non-reservation loop, `>` in the fold (the least time wins), reservation jobs that ignore node events, get_if that skips pending
references.  Python integers: nothing overflows; absl::Time's saturation is written out."""
from __future__ import annotations

import numpy as np

from cranesched_amd import abi

I64_MAX, I64_MIN = (1 << 63) - 1, -(1 << 63)


def _time_add(t: int, d: int) -> int:
    """absl::Time + absl::Duration saturates at InfiniteFuture / InfinitePast (job->end_time = start_time + time_limit, :6772)."""
    return max(I64_MIN, min(I64_MAX, t + d))


def check(start_sec, reason, place_offsets, node_idx, events: "abi.CommitEvents | None", jobs: abi.CommitJobs):
    """-> (code uint8 [J], counts uint64 [8])"""
    J = jobs.num_jobs
    ev = events if events is not None else abi.CommitEvents()
    craned_id_change_time_map: dict = {}                                             # :1466
    affected_resv_set: dict = {}                                                     # :1467 (value: the entry's position)
    for a, rid in enumerate(ev.ar_resv.tolist()):                                    # :1470-1472 holds_alternative<ResvId>
        affected_resv_set[rid] = a
    for e, end_time in enumerate(ev.ev_time_sec.tolist()):                           # :1473-1477
        for craned_id in ev.ev_nodes[int(ev.ev_offsets[e]):int(ev.ev_offsets[e + 1])].tolist():   # :1478
            it = craned_id_change_time_map.get(craned_id)                            # :1479
            if it is None or it > end_time:                                          # :1480-1481
                craned_id_change_time_map[craned_id] = end_time                      # :1482
    code = np.zeros(J, np.uint8)
    for j in range(J):                                                               # :1492
        if jobs.gone is not None and jobs.gone[j]:                                   # :1493-1500 not in the pending map: continue
            code[j] = abi.COMMIT_GONE
            continue
        if int(reason[j]) != 0:                                                      # :1507-1510 !reason.empty(): continue
            code[j] = abi.COMMIT_NOT_STARTED
            continue
        end_time = _time_add(int(start_sec[j]), int(jobs.time_limit_sec[j]))         # :1511
        craned_ids = [n for n in node_idx[int(place_offsets[j]):int(place_offsets[j + 1])].tolist() if n != abi.NODE_NONE]
        resv = abi.RESV_NONE if jobs.reservation is None else int(jobs.reservation[j])
        why = abi.COMMIT_OK
        if resv == abi.RESV_NONE:                                                    # :1512 reservation.empty()
            for craned_id in craned_ids:                                             # :1514 (no break)
                it = craned_id_change_time_map.get(craned_id)                        # :1515
                if it is not None and it < end_time:                                 # :1516-1517
                    why = abi.COMMIT_RESOURCE_CHANGED                                # :1518
        elif resv in affected_resv_set:                                              # :1521
            a = affected_resv_set[resv]                                              # :1522-1523 GetResvMetaPtr, NOW
            if not ev.ar_exists[a]:                                                  # :1524
                why = abi.COMMIT_RESV_DELETED                                        # :1525
            elif int(ev.ar_end_sec[a]) < end_time:                                   # :1526
                why = abi.COMMIT_RESV_ENDS_EARLY                                     # :1527
            else:
                now_ids = set(ev.ar_nodes[int(ev.ar_offsets[a]):int(ev.ar_offsets[a + 1])].tolist())
                for craned_id in craned_ids:                                         # :1529
                    if craned_id not in now_ids:                                     # :1530
                        why = abi.COMMIT_RESV_CHANGED                                # :1531
                        break                                                        # :1532
        if why != abi.COMMIT_OK:                                                     # :1537-1540
            code[j] = why
            continue
        preempted_still_alive = False                                                # :1542
        if jobs.preempt_offsets is not None:
            for ref in jobs.preempted[int(jobs.preempt_offsets[j]):int(jobs.preempt_offsets[j + 1])].tolist():   # :1543
                if ref & abi.PREEMPT_REF_PENDING:                                    # :1544-1545 get_if<RnJobInScheduler*>: a pending one is skipped
                    continue
                if jobs.running_alive[ref]:                                          # :1546
                    preempted_still_alive = True                                     # :1547
                    break                                                            # :1548
        if preempted_still_alive:                                                    # :1551
            code[j] = abi.COMMIT_WAITING_PREEMPTION                                  # :1552
            continue
        code[j] = abi.COMMIT_OK                                                      # reaches :1557
    return code, np.bincount(code, minlength=8).astype(np.uint64)
