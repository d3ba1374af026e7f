"""GpuNodeSelectionAlgo::CommitCheck (cranesched_amd/host) through its driver, host/test_commit_adapter: a hand-made string-level cycle,
the reason strings of JobScheduler.cpp:1518-1552 in job->reason, unknown craned and reservation names dropped, a cycle with preemption,
and CheckAndMallocMetaResource behind it skipping the dropped jobs — all written out in the driver.  A fresh child process under a time
limit of its own."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "cranesched_amd", "host", "test_commit_adapter")


def test_no_device_is_loud(built):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    r = subprocess.run([DRIVER, "--no-gpu"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "no device: CommitCheck refuses with status -2" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_commit_check_on_a_hand_made_cycle(gpu):
    r = subprocess.run([DRIVER], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "hand cases: 0 failures" in r.stdout, r.stdout + r.stderr
