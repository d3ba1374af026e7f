"""cns_running_amend_ends (include/crane_gpu_amend/running_amend.h) in plain Python over tests/running_pyref.py's Ledger: every row whose
id is listed gets the listed end; nothing else moves.  What a cycle makes of the amended ledger comes from the existing yardsticks
(cns_set_running and the oracle) fed with Ledger.arrays() — never from the code under test."""
from __future__ import annotations

import numpy as np

from tests import running_pyref as rp


def amend(led: "rp.Ledger", job_ids, end_sec):
    """-> (found per id, rows written); `led` is changed in place.  An id no row carries changes nothing
    (ERR_NON_EXISTENT, JobScheduler.cpp:2302-2305)."""
    ids = [int(i) for i in job_ids]
    ends = [int(e) for e in end_sec]
    assert len(ids) == len(ends) and len(set(ids)) == len(ids), "one end per id, ids distinct"
    assert all(rp.I64_MIN <= e <= rp.I64_MAX for e in ends)
    new = dict(zip(ids, ends))
    have = set()
    written = 0
    for r in led.rows:
        if r.job_id in new:
            r.end_sec = new[r.job_id]
            have.add(r.job_id)
            written += 1
    return np.array([1 if i in have else 0 for i in ids], np.uint8), written
