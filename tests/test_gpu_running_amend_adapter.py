"""GpuNodeSelectionAlgo::AmendRunning and QueryReservation on the device ledger (cranesched_amd/host) through their driver,
host/test_running_amend_adapter: three consecutive cycles through NodeSelect on a cluster with shared nodes and a reservation; between
them a time-limit change on a running job, an array parent's two running children in one call and a resume that extends an end — once
with the running set handed in every cycle (the new ends written into the RnJobInScheduler objects), once resident through
AmendRunning.  Every job's reason, start, nodes and allocated cores and every answer of QueryReservation must be identical, and differ
from a run that forgets the amendments.  A fresh child process under a time limit of its own."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "cranesched_amd", "host", "test_running_amend_adapter")


def test_no_device_is_loud(built):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    r = subprocess.run([DRIVER, "--no-gpu"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "no device: AmendRunning refuses with status -2" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_three_cycles_amended_resident_and_handed_in(gpu):
    r = subprocess.run([DRIVER], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "hand cases: 3 cycles, 4 rows amended" in r.stdout and " 0 differ; " in r.stdout and " 0 failures" in r.stdout, r.stdout + r.stderr
