"""The input rules of cns_gate_pending (cranesched_amd/csrc/gate_check_host.inc, no HIP in there) compiled with g++ and driven by
tests/cpp/gate_host_test.cpp: every CNS_ERR_INVALID_ARG rule of include/crane_gpu_gate/pending_gate.h by its message, the size limits,
and what a valid call reports.  The same stand-alone program is built a second time with -fsanitize=address,undefined and run over the
same cases (its arrays are exactly as long as the header says).  No GPU involved, nothing loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "gate_host_test.cpp")

WANT = {
    "valid": (0, "J=4 D=5 E=2 deps=1 array=1"),
    "valid_no_events": (0, "J=4 D=5 E=0 deps=1 array=1"),
    "valid_bare": (0, "J=4 D=0 E=0 deps=0 array=0"),
    "valid_empty": (0, "J=0 D=0 E=2 deps=0 array=0"),
    "valid_offsets_without_entries": (0, "J=4 D=0 E=2 deps=1 array=1"),
    "list_border_is_free": (0, "J=4 D=5 E=2 deps=1 array=1"),
    "no_job_id": (-1, "cns_gate_pending: missing array: job_id"),
    "no_code": (-1, "cns_gate_pending: missing array: out->code or out->pending"),
    "no_pending": (-1, "cns_gate_pending: missing array: out->code or out->pending"),
    "no_num_pending": (-1, "cns_gate_pending: missing array: out->num_pending"),
    "no_event_sec": (-1, "cns_gate_pending: events with a missing array"),
    "no_event_dependee": (-1, "cns_gate_pending: events with a missing array"),
    "is_or_without_ready": (-1, "cns_gate_pending: dep_is_or and dep_ready_sec come together"),
    "ready_without_is_or": (-1, "cns_gate_pending: dep_is_or and dep_ready_sec come together"),
    "entries_without_dep_job": (-1, "cns_gate_pending: dependency entries with a missing array (dep_is_or, dep_ready_sec, dep_job, dep_delay_sec)"),
    "entries_without_delay": (-1, "cns_gate_pending: dependency entries with a missing array (dep_is_or, dep_ready_sec, dep_job, dep_delay_sec)"),
    "entries_without_is_or": (-1, "cns_gate_pending: dependency entries with a missing array (dep_is_or, dep_ready_sec, dep_job, dep_delay_sec)"),
    "ap_without_flags": (-1, "cns_gate_pending: array_parent with a missing ap_ array"),
    "ap_without_deadline": (-1, "cns_gate_pending: array_parent with a missing ap_ array"),
    "ap_without_running": (-1, "cns_gate_pending: array_parent with a missing ap_ array"),
    "ap_without_limit": (-1, "cns_gate_pending: array_parent with a missing ap_ array"),
    "job_id_equal": (-1, "cns_gate_pending: job_id is not strictly ascending at row 2"),
    "job_id_descends": (-1, "cns_gate_pending: job_id is not strictly ascending at row 3"),
    "offsets_first": (-1, "cns_gate_pending: dep_offsets[0] != 0"),
    "offsets_decrease": (-1, "cns_gate_pending: dep_offsets decrease at job 1"),
    "list_equal": (-1, "cns_gate_pending: the dependency list of row 0 is not strictly ascending at entry 1"),
    "list_descends": (-1, "cns_gate_pending: the dependency list of row 2 is not strictly ascending at entry 3"),
    "flags_outside": (-1, "cns_gate_pending: ap_flags[0] has a bit outside CNS_GATE_AP_*"),
    "too_many_jobs": (-4, "cns_gate_pending: more than 2^32 - 512 jobs"),
    "jobs_at_the_limit_reach_the_arrays": (-1, "cns_gate_pending: missing array: job_id"),
    "too_many_events": (-4, "cns_gate_pending: more than 2^32 - 256 events"),
    "too_many_entries": (-4, "cns_gate_pending: more than 2^32 - 256 dependency entries"),
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


def test_every_rule_by_its_message(tmp_path):
    _check(_build(tmp_path, "gate_host_test", []))


def test_the_same_cases_under_address_and_ub_sanitizers(tmp_path):
    """A stand-alone program with its own main: the sanitizer runtime is linked in, nothing is preloaded."""
    exe = _build(tmp_path, "gate_host_test_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    _check(exe)
