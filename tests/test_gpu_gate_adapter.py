"""GpuNodeSelectionAlgo::BuildPendingQueue (cranesched_amd/host) through its driver, host/test_gate_adapter, on a 2 000-job pending map in
CraneCtld's shapes over two cycles, the second fed with the DependenciesInJob the first wrote back.  The driver compares against its
own serial restatement of JobScheduler.cpp:1353-1413; here what it dumps — both cycles' inputs and what the adapter left behind — is held
against tests/gate_pyref.py: codes, pending_jobs, and every job's final deps / ready_time.  A fresh child process under a time limit of
its own."""
import os
import subprocess

import pytest

from tests import gate_pyref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "cranesched_amd", "host", "test_gate_adapter")


def test_no_device_is_loud(built):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    r = subprocess.run([DRIVER, "--no-gpu"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "no device: BuildPendingQueue refuses with status -2" in r.stdout, r.stdout + r.stderr


def _parse(path):
    """-> [cycle]: now, jobs (ref.Job, in the driver's order), events, results {id: (code, ready, sorted deps left)}, pending [(id, array?)], stats"""
    cycles = []
    for line in open(path):
        w = line.split()
        if w[0] == "cycle":
            cycles.append(dict(now=int(w[3]), jobs=[], events=[], results={}, pending=[], stats=None))
            continue
        c = cycles[-1]
        if w[0] == "job":
            (jid, held, begin, is_or, ready, is_ap, meta, parent, complete, cancel, deadline, has_next, running, limit, n) = (int(x) for x in w[1:16])
            deps = {int(k): int(d) for k, d in (e.split(":") for e in w[16:16 + n])}
            ap = ref.ArrayParent(bool(meta), bool(parent), bool(complete), bool(cancel), deadline, bool(has_next), running, limit) if is_ap else None
            c["jobs"].append(ref.Job(jid, bool(held), begin, ref.Dependencies(deps, bool(is_or), ready), ap))
        elif w[0] == "event":
            c["events"].append((int(w[1]), int(w[2]), int(w[3])))
        elif w[0] == "result":
            c["results"][int(w[1])] = (int(w[2]), int(w[3]), sorted(int(x) for x in w[5:5 + int(w[4])]))
        elif w[0] == "pending":
            c["pending"] = [(int(a), int(b)) for a, b in (e.split(":") for e in w[1:])]
        elif w[0] == "stats":
            c["stats"] = [int(x) for x in w[1:4]]
    return cycles


@pytest.mark.gpu
def test_build_pending_queue_over_two_cycles(gpu, tmp_path):
    dump = tmp_path / "gate_adapter.txt"
    r = subprocess.run([DRIVER, "2000", "--dump", str(dump)], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "gate cases: 0 failures" in r.stdout, r.stdout + r.stderr
    cycles = _parse(dump)
    assert len(cycles) == 2 and all(len(c["jobs"]) == 2000 == len(c["results"]) for c in cycles)
    carried = None   # the restatement's own jobs after cycle 0: what the reference's JobInCtld would hold
    for n, c in enumerate(cycles):
        jobs = c["jobs"]
        if carried is not None:   # the adapter's write-back IS the next input: the dump's second cycle must start where the restatement stands
            for j in jobs:
                w = carried[j.job_id].dependencies
                assert (j.dependencies.deps, j.dependencies.ready_time, j.dependencies.is_or) == (w.deps, w.ready_time, w.is_or), f"cycle {n} input, job {j.job_id}"
        res = ref.gate(c["now"], jobs, c["events"])            # mutates `jobs` as the reference mutates its JobInCtld
        by_id = sorted(jobs, key=lambda j: j.job_id)
        assert len(set(res.code.tolist())) >= 6, "the case reaches both OK kinds and every gate in front of the array parent's"
        for row, j in enumerate(by_id):
            code, ready, left = c["results"][j.job_id]
            assert code == int(res.code[row]), f"cycle {n}, job {j.job_id}"
            assert (ready, left) == (j.dependencies.ready_time, sorted(j.dependencies.deps)), f"cycle {n}, job {j.job_id}: the write-back"
        want_pending = [(by_id[int(r)].job_id, int(m)) for r, m in zip(res.pending, res.materializes)]
        assert c["pending"] == want_pending, f"cycle {n}: pending_jobs"
        assert c["stats"] == res.ev_stats.tolist() and c["stats"][0] > 100 and c["stats"][1] > 0 and c["stats"][2] > 0
        carried = {j.job_id: j for j in jobs}
