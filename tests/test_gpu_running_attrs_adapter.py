"""The adapter's side of include/crane_gpu_running/running_attrs.h through its driver, host/test_running_attrs_adapter: a
GpuMultiFactorPriority that borrows the GpuNodeSelectionAlgo's engine ranks the pending queue from the device ledger — with
`running_jobs` handed in EMPTY, so nothing of the vector is read — and gives the order, and the priorities bit for bit, of a
GpuMultiFactorPriority of its own fed the same running jobs in ledger order, over four cycles with jobs ending and starting and a new
snapshot in between.  A fresh child process under a time limit of its own."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "cranesched_amd", "host", "test_running_attrs_adapter")


def test_no_device_is_loud(built):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    r = subprocess.run([DRIVER, "--no-gpu"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "no device: the borrowed sorter refuses" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_the_borrowed_sorter_ranks_from_the_ledger(gpu):
    r = subprocess.run([DRIVER], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "attrs adapter: 4 cycles" in r.stdout and "0 orders or priorities differ, 0 failures" in r.stdout, r.stdout + r.stderr
