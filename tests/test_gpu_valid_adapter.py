"""GpuNodeSelectionAlgo::CheckJobValidity (cranesched_amd/host) through its driver, host/test_valid_adapter: a hand-made string-level
cluster, the expected codes, eligible counts and CraneErrCode names written out in the driver.  A fresh child process under a time limit
of its own."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "cranesched_amd", "host", "test_valid_adapter")


def test_no_device_is_loud(built):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    r = subprocess.run([DRIVER, "--no-gpu"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "no device: CheckJobValidity refuses with status -2" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_check_job_validity_on_a_hand_made_cluster(gpu):
    r = subprocess.run([DRIVER], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and ", 0 failures" in r.stdout, r.stdout + r.stderr
