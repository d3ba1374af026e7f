"""GpuNodeSelectionAlgo with UseResidentRunning(true) and a snapshot that has preempt_enabled (cranesched_amd/host) through its driver,
host/test_running_preempt_adapter, without --bench: three consecutive cycles with preemption through NodeSelect on a crowded cluster
with shared nodes and a reservation, a craned state flip in between, each cycle built from the previous one's results — once with the
running set handed in every cycle (cns_set_running + cns_select_preempt), once with it kept on the device
(cns_running_select_preempt).  Every job's reason, start, nodes, allocated cores and preempted list, the cancelled ids and the
preempting set must be identical.  A fresh child process under a time limit of its own."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "cranesched_amd", "host", "test_running_preempt_adapter")


def test_no_device_is_loud(built):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    r = subprocess.run([DRIVER, "--no-gpu"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "no device: NodeSelect refuses with status -2" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_three_cycles_with_preemption_resident_and_handed_in(gpu):
    r = subprocess.run([DRIVER], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "hand cases: 3 cycles with preemption" in r.stdout and "0 lines differ, 0 failures" in r.stdout, r.stdout + r.stderr
