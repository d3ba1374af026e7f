"""The launch plan of a cycle (cranesched_amd/csrc/plan_host.inc: the partitions of the a / b / c launches, per launch the ordered candidates
k_wide -> k_pipe -> k_select or k_giant -> k_mem with build, tile width, extra home / helper workgroups and grid, the meaning of every
CNS_SELECT_KERNEL value against cns_config::kernel_pin, what the retry after a protocol fault may use, and the bytes of
cns_debug_last_kernel) compiled with g++ and held to the engine's rules row by row (tests/cpp/plan_host_test.cpp).  No GPU involved: the
plan is arithmetic on the build's figures, which the test writes out as literals and engine.hip static_asserts against its constants."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def plan_host(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("plan_host") / "plan_host_test")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "plan_host_test.cpp")], check=True)
    return exe


def test_launch_plan_follows_the_engines_rules(plan_host):
    r = subprocess.run([plan_host], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
