"""The input rules of cns_running_seed / cns_running_advance (cranesched_amd/csrc/running_check_host.inc, no HIP in there) compiled with
g++ and driven by tests/cpp/running_host_test.cpp: every refusal of include/crane_gpu_running/running.h by its status and message, the
size limits, and what a valid call reports (the retire ids sorted, and where each came from).  The same stand-alone program is built a
second time with -fsanitize=address,undefined and run over the same cases (its arrays are exactly as long as the header says).  No GPU
involved, nothing loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "running_host_test.cpp")

MISSING = (-1, "cns_running_seed: missing array")
SORTED = (0, "sorted=3,9,12, order=1,0,2,")
WANT = {
    "seed_valid": (0, "R=3 A=3"),
    "seed_null_set": (0, "R=0 A=0"),
    "seed_no_jobs": (0, "R=0 A=0"),
    "seed_no_end": MISSING, "seed_no_offsets": MISSING, "seed_no_node": MISSING, "seed_no_cpu": MISSING, "seed_no_mem": MISSING,
    "seed_no_core_lo": MISSING,
    "seed_no_ids": (-1, "cns_running_seed: missing array: job_ids"),
    "seed_num_allocs": (-1, "cns_running_seed: num_allocs mismatch"),
    "seed_offsets_first": (-1, "cns_running_seed: alloc_offsets[0] != 0"),
    "seed_offsets_decrease": (-1, "cns_running_seed: alloc_offsets decrease at job 1"),
    "seed_node_outside": (-1, "running allocation on node >= num_nodes"),   # build_running's own words
    "seed_node_at_the_border": (0, "R=3 A=3"),
    "seed_id_twice": (-1, "cns_running_seed: job id 7 stands twice in job_ids"),
    "seed_too_many_jobs": (-4, "cns_running_seed: more than 2^32 - 512 jobs"),
    "seed_too_many_allocs": (-4, "cns_running_seed: more than 2^32 - 256 allocations"),
    "step_valid": SORTED,
    "step_empty": (0, "sorted= order="),
    "step_retire_only": SORTED,
    "step_admit_all": (0, "sorted= order="),
    "step_no_ledger": (-5, "cns_running_advance before cns_running_seed (cns_set_running and a changed num_nodes drop the ledger)"),
    "step_no_retire_ids": (-1, "cns_running_advance: missing array: retire_ids"),
    "step_no_found": (-1, "cns_running_advance: missing array: out->found"),
    "step_no_out": (-1, "cns_running_advance: missing array: out->found"),
    "step_retire_twice": (-1, "cns_running_advance: job id 9 stands twice in retire_ids"),
    "step_no_cycle": (-5, "cns_running_advance: the admit step needs the results of a successful cycle"),
    "step_preempt_cycle": (-5, "cns_running_advance: the admit step is not served after cns_select_preempt"),
    "step_other_queue": (-1, "cns_running_advance: num_jobs 4 is not the last cycle's 5"),
    "step_other_now": (-1, "cns_running_advance: now_sec 999 is not the last cycle's 1000"),
    "step_no_job_id": (-1, "cns_running_advance: missing array: job_id"),
    "step_too_many_retire": (-4, "cns_running_advance: more than 2^32 - 256 retire ids"),
    "step_too_many_jobs": (-4, "cns_running_advance: more than 2^32 - 512 jobs in the ledger"),
    "step_jobs_at_the_limit": SORTED,
    "step_too_many_allocs": (-4, "cns_running_advance: more than 2^32 - 256 allocations in the ledger"),
    "pairs_fit": (0, ""),
    "pairs_no_slot_at_all": (0, ""),
    "pairs_too_many": (-4, "the running set's allocations times the slots of the node in most partitions exceed 2^32 - 256"),
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
    _check(_build(tmp_path, "running_host_test", []))


def test_the_same_cases_under_address_and_ub_sanitizers(tmp_path):
    """A stand-alone program with its own main: the sanitizer runtime is linked in, nothing is preloaded."""
    exe = _build(tmp_path, "running_host_test_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    _check(exe)
