"""The input rules of cns_running_amend_ends (cranesched_amd/csrc/running_amend_check_host.inc, no HIP in there) compiled with g++ and
driven by tests/cpp/running_amend_host_test.cpp: every refusal of include/crane_gpu_amend/running_amend.h by its status and message,
the limit of 2^32 - 256 amendments, and what a valid call reports (the ids sorted, their ends beside them, and where each came from).
The same stand-alone program is built a second time with -fsanitize=address,undefined and run over the same cases (its arrays are
exactly as long as the header says).  No GPU involved, nothing loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "running_amend_host_test.cpp")

I64_MAX, I64_MIN = (1 << 63) - 1, -(1 << 63)
SORTED = (0, f"sorted=0,9,12,4294967295, ends={I64_MAX},900,{I64_MIN},-5, order=2,0,3,1,")
NO_LEDGER = (-5, "cns_running_amend_ends before cns_running_seed (cns_set_running and a changed num_nodes drop the ledger)")
WANT = {
    "valid": SORTED,
    "one": (0, "sorted=5, ends=77, order=0,"),
    "descending": (0, "sorted=10,20,30, ends=1,2,3, order=2,1,0,"),
    "empty": (0, "sorted= ends= order="),
    "no_count_wanted": SORTED,
    "no_ledger": NO_LEDGER,
    "no_ledger_and_empty": NO_LEDGER,
    "no_ids": (-1, "cns_running_amend_ends: missing array: job_ids"),
    "no_ends": (-1, "cns_running_amend_ends: missing array: end_sec"),
    "no_found": (-1, "cns_running_amend_ends: missing array: out->found"),
    "no_out": (-1, "cns_running_amend_ends: missing array: out->found"),
    "id_twice": (-1, "cns_running_amend_ends: job id 3 stands twice in job_ids"),
    "id_zero_twice": (-1, "cns_running_amend_ends: job id 0 stands twice in job_ids"),
    "too_many": (-4, "cns_running_amend_ends: more than 2^32 - 256 amendments"),
    "at_the_limit": (-1, "cns_running_amend_ends: missing array: job_ids"),   # past the limit's rule, stopped by the next one
}


def _build(tmp, name, extra):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp / name)
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", *extra, "-o", exe, SRC], check=True)
    return exe


def _check(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    got = {}
    for line in r.stdout.splitlines():
        name, rest = line.split(": ", 1)
        status, _, msg = rest.partition(" ")
        got[name] = (int(status), msg)
    assert sorted(got) == sorted(WANT), "every case ran"
    for name, want in WANT.items():
        assert got[name] == want, name
    assert r.stderr == ""


def test_every_rule_by_its_status_and_message(tmp_path):
    _check(_build(tmp_path, "running_amend_host_test", []))


def test_the_same_cases_under_address_and_ub_sanitizers(tmp_path):
    """A stand-alone program with its own main: the sanitizer runtime is linked in, nothing is preloaded."""
    exe = _build(tmp_path, "running_amend_host_test_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    _check(exe)
