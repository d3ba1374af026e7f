#!/usr/bin/env python3
"""What-if probes (include/crane_gpu_probe/probe.h): device time of k_probe behind one full-size cycle, per batch size Q.
   python tools/probe_bench.py [--config C4] [--qs 1,64,4096,65536] [--runs 5] [--mem-jobs 20000]      -> one JSON line
Per Q also the wall time of the three calls on the host (`call_ms`: cns_probe_upload, cns_probe_run_resident, cns_probe_download; medians
of --runs rounds) — what a change to the host side of the probes is compared by.
Beside every figure the two things it is to be read against, measured in the same process:
  (a) cycle_ms      the cycle itself — before the probes, the only way to one answer was another cycle with the job appended;
  (b) k_mem_us_per_decision   the sequential form of the same walk (one workgroup, every job scans its partition's slots in HBM):
      CNS_SELECT_KERNEL=mem on a prefix of the same queue on the same cluster.
Run each configuration as a process of its own, under its own time limit."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from cranesched_amd import synth
from cranesched_amd.engine import GpuNodeSelector

ap = argparse.ArgumentParser()
ap.add_argument("--config", default="C4")
ap.add_argument("--jobs", type=int, default=None)
ap.add_argument("--nodes", type=int, default=None)
ap.add_argument("--qs", default="1,64,4096,65536")
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--mem-jobs", type=int, default=20000)
a = ap.parse_args()

cfg = synth.CONFIGS[a.config]
cluster, jobs, now = synth.make_config(a.config, J=a.jobs, N=a.nodes)
P = cluster.num_partitions
eng = GpuNodeSelector()
eng.set_nodes(cluster)
eng.upload_jobs(jobs)
eng.run_resident(now)                                   # warm-up
cyc = []
for _ in range(3):
    eng.run_resident(now)
    cyc.append(eng.timing()["select_ms"] + eng.timing()["init_ms"])
out = {"config": a.config, "jobs": jobs.num_jobs, "nodes": cluster.num_nodes, "partitions": P, "kernel": eng.last_kernel(),
       "cycle_ms": float(np.median(cyc)), "probes": []}
cycle_results = eng.download()
for Q in [int(x) for x in a.qs.split(",")]:
    probes = synth.make_jobs(Q, P, cfg["gres"], synth.SEED0 ^ 0x50524F42, cfg["Q"], cfg["LM"])
    eng.probe_upload(probes)
    eng.probe_run_resident()                            # warm-up (scratch buffers)
    ms = [eng.probe_run_resident() for _ in range(max(a.runs, 5))]
    got = eng.probe_download()
    m = float(np.median(ms))
    wall = []                                           # one round: upload, run, download, each timed on its own
    for _ in range(max(a.runs, 5)):
        t = [time.perf_counter()]
        for call in (lambda: eng.probe_upload(probes), eng.probe_run_resident, eng.probe_download):
            call()
            t.append(time.perf_counter())
        wall.append(np.diff(t) * 1e3)
    up, run, down = (float(x) for x in np.median(wall, axis=0))
    r, s = got.reason[:Q], got.start_sec[:Q]
    out["probes"].append({"Q": Q, "kernel_ms": m, "min_ms": float(min(ms)), "max_ms": float(max(ms)), "us_per_probe": 1e3 * m / Q,
                          "probes_per_s": Q / (m * 1e-3), "start_now": int(((r == 0) & (s == now)).sum()), "later": int((s > now).sum()),
                          "no_start": int((s == 0).sum()), "call_ms": {"upload": up, "run_resident": run, "download": down}})
assert eng.download().diff(cycle_results) is None, "the cycle's results changed under the probe calls"
eng.close()
# (b) the same walk, sequential: k_mem on a prefix of the queue
if a.mem_jobs:
    os.environ["CNS_SELECT_KERNEL"] = "mem"
    cm, jm, _ = synth.make_config(a.config, J=min(a.mem_jobs, jobs.num_jobs), N=a.nodes)
    e2 = GpuNodeSelector()
    e2.set_nodes(cm)
    e2.upload_jobs(jm)
    e2.run_resident(now)
    t = []
    for _ in range(3):
        e2.run_resident(now)
        t.append(e2.timing()["select_ms"])
    out["k_mem"] = {"jobs": jm.num_jobs, "kernel": e2.last_kernel(), "select_ms": float(np.median(t)),
                    "us_per_decision": 1e3 * float(np.median(t)) / jm.num_jobs, "chains": P,   # (P workgroups side by side, one per partition)
                    "us_per_decision_of_one_chain": 1e3 * float(np.median(t)) * P / jm.num_jobs}
    e2.close()
print(json.dumps(out))
