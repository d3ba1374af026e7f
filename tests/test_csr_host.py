"""The CSR rules of the callers' lists (cranesched_amd/csrc/csr_host.inc: an offsets array starts at 0 and never decreases; a list, once
sorted, names no value twice and none at or above a bound) compiled with g++ and held to hand cases and to the standard library's own
sort / adjacent_find / max_element over seeded random CSRs (tests/cpp/csr_host_test.cpp).  No GPU involved."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def csr_host(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("csr_host") / "csr_host_test")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "csr_host_test.cpp")], check=True)
    return exe


def test_csr_checks_agree_with_the_standard_library(csr_host):
    r = subprocess.run([csr_host], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
