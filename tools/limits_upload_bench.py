"""Host cost of cns_upload_limit_jobs at C4's queue (1 M jobs): the wall time of the call through the binding, its HIP-event time (the
uploads and allocations between the call's two events), and the rest: the validating pass over the keys and the call's fixed cost.
12 calls, the first 2 dropped.  Prints one JSON line (profiles/r19_acct_space.txt)."""
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from cranesched_amd import synth
from cranesched_amd.engine import GpuNodeSelector

cluster, jobs, now = synth.make_config("C4")
tables, lim_jobs = synth.make_limits("C4", cluster, jobs)
eng = GpuNodeSelector(device=0)
eng.set_nodes(cluster)
eng.upload_jobs(jobs)
eng.set_run_limits(tables)
cj = lim_jobs.to_c()
wall, ev = [], []
for i in range(12):
    t0 = time.perf_counter()
    rc = eng._L.cns_upload_limit_jobs(eng._h, C.byref(cj))
    t1 = time.perf_counter()
    assert rc == 0
    wall.append((t1 - t0) * 1e3)
    ev.append(eng.limit_timing()["h2d_ms"])
eng.close()
wall, ev = np.array(wall[2:]), np.array(ev[2:])
print(json.dumps({"jobs": int(lim_jobs.num_jobs), "calls": len(wall), "wall_ms_median": round(float(np.median(wall)), 4),
                  "event_ms_median": round(float(np.median(ev)), 4), "host_rest_ms_median": round(float(np.median(wall - ev)), 4),
                  "host_rest_ms_all": [round(float(x), 4) for x in wall - ev]}))
