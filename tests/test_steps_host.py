"""The host pass of cns_schedule_steps (cranesched_amd/csrc/steps_host.inc: every argument check and the re-layout of the caller's arrays into
one record per step and one Res per (job, node)) and the step scheduler's top-k queue (cranesched_amd/csrc/step_pq.h), compiled with g++ and
held to hand-written records, to one input per refusal, and to the real std::priority_queue, by tests/cpp/steps_host_test.cpp.  No GPU
involved: what this routine lets through is what k_sched_steps indexes without a bound check of its own, so the refusals are tested here and
never by handing the device a bad input.  The same program runs once more under AddressSanitizer and UBSan: it is host code with its own main."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "steps_host_test.cpp")


def _build(tmp_path_factory, name, extra):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp(name) / name)
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", *extra, "-o", exe, SRC], check=True)
    return exe


@pytest.fixture(scope="module")
def steps_host(tmp_path_factory):
    return _build(tmp_path_factory, "steps_host_test", [])


@pytest.fixture(scope="module")
def steps_host_sanitised(tmp_path_factory):
    return _build(tmp_path_factory, "steps_host_test_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def test_step_records_refusals_and_queue(steps_host):
    r = subprocess.run([steps_host], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_step_records_refusals_and_queue_sanitised(steps_host_sanitised):
    r = subprocess.run([steps_host_sanitised], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
