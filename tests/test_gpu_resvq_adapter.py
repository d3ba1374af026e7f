"""GpuNodeSelectionAlgo::QueryReservation (cranesched_amd/host) through its driver, host/test_resv_adapter: four hand-made
string-level clusters, the expected answers written out in the driver.  A fresh child process under a time limit of its own."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "cranesched_amd", "host", "test_resv_adapter")


def test_no_device_is_loud(built):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    r = subprocess.run([DRIVER, "--no-gpu"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "ok (no device" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_query_reservation_on_hand_made_clusters(gpu):
    r = subprocess.run([DRIVER], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "ok: QueryReservation on 4 hand-made clusters" in r.stdout, r.stdout + r.stderr
