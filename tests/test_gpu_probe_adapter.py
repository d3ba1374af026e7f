"""GpuNodeSelectionAlgo::ProbeStart (cranesched_amd/host): the driver test_probe_adapter compares every probe with what the adapter's
own cycle path writes for the same job appended to the same queue."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "cranesched_amd", "host", "test_probe_adapter")


def test_probe_adapter_without_gpu_is_loud(built):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    r = subprocess.run([EXE, "--no-gpu"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr


@pytest.mark.gpu
def test_probe_start_equals_the_cycle_path_on_gpu(built, monkeypatch):
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "32 of 32 probes identical" in r.stdout
