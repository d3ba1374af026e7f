"""The pass count of the segment half of cns_resvq_run's sort (cranesched_amd/csrc/resvq_passes.inc) compiled with g++ and held to
its definition on both sides of every query count at which it changes (tests/cpp/resvq_passes_test.cpp): plain, and once under
AddressSanitizer + UndefinedBehaviorSanitizer as an executable of its own.  No GPU involved."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "resvq_passes_test.cpp")


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def passes_exe(tmp_path_factory, request):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("resvq_passes_" + request.param) / "resvq_passes_test")
    extra = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "sanitized" else []
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", *extra, "-o", exe, SRC], check=True)
    return exe


def test_pass_count_holds_every_segment_number(passes_exe):
    r = subprocess.run([passes_exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_the_host_uses_the_routine():
    """resvq_host.inc takes its pass count from the routine under test, not from a loop of its own."""
    host = open(os.path.join(ROOT, "cranesched_amd", "csrc", "resvq_host.inc")).read()
    assert "cns_resvq::seg_passes(Q)" in host and "++seg_passes" not in host
    assert '#include "resvq_passes.inc"' in open(os.path.join(ROOT, "cranesched_amd", "csrc", "engine.hip")).read()
