"""The input rules of cns_running_select_preempt and of the admit step behind it (cranesched_amd/csrc/running_preempt_check_host.inc, no
HIP in there) compiled with g++ and driven by tests/cpp/running_preempt_host_test.cpp: every refusal of
include/crane_gpu_running/running_preempt.h by its status and message, the size limits, and what a valid call reports (the preempting
ids ascending, each once).  The same stand-alone program is built a second time with -fsanitize=address,undefined and run over the same
cases (its arrays are exactly as long as the header says).  No GPU involved, nothing loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "running_preempt_host_test.cpp")

OK = (0, "set=3,4,9,")
NULL = (-1, "cns_running_select_preempt: null argument")
PENDING = (-1, "cns_running_select_preempt: missing pending-job array")
RUNNING = (-1, "cns_running_select_preempt: missing running-job array")
OUTPUT = (-1, "cns_running_select_preempt: missing output array")
QOS = (-1, "cns_running_select_preempt: missing array: the QoS preempt lists")
WANT = {
    "call_valid": OK,
    "call_no_jobs_arg": NULL, "call_no_preempt_arg": NULL, "call_no_out_arg": NULL, "call_no_pout_arg": NULL,
    "call_no_nodes": (-5, "cns_running_select_preempt before cns_set_nodes"),
    "call_no_ledger": (-5, "cns_running_select_preempt before cns_running_seed (cns_set_running and a changed num_nodes drop the ledger)"),
    "call_tables_not_the_ledgers": (-5, "cns_running_select_preempt: the per-slot running tables are not the ledger's (cns_set_nodes / cns_set_reservations "
                                        "emptied them: call cns_running_advance first)"),
    "call_too_many_pending": (-4, "cns_running_select_preempt: 2^31 pending jobs or more (bit 31 of a reference marks a pending job)"),
    "call_pending_at_the_limit": OK,
    "call_too_many_rows": (-4, "cns_running_select_preempt: 2^31 ledger rows or more (bit 31 of a reference marks a pending job)"),
    "call_no_pd_qos": PENDING, "call_no_pd_qos_priority": PENDING, "call_no_pd_priority": PENDING,
    "call_empty_queue_needs_no_pending_array": OK,
    "call_no_rn_job_id": RUNNING, "call_no_rn_qos": RUNNING, "call_no_rn_qos_priority": RUNNING, "call_no_rn_start": RUNNING,
    "call_empty_ledger_needs_no_running_array": OK,
    "call_no_qos_offsets": QOS, "call_no_qos_lists": QOS,
    "call_empty_qos_lists_need_no_array": OK,
    "call_no_set": (-1, "cns_running_select_preempt: missing array: preempting_job_ids"),
    "call_empty_set": (0, "set="),
    "call_no_offsets_out": OUTPUT, "call_no_preempted_out": OUTPUT, "call_no_cancelled_out": OUTPUT, "call_no_preempting_out": OUTPUT,
    "row_id": (-1, "cns_running_select_preempt: rn_job_id[2] is 9, ledger row 2 carries job id 8 (the running-job arrays are in ledger order)"),
    "admit_mask_given": (0, ""),
    "admit_no_mask": (-1, "cns_running_advance: missing array: admit (required after cns_running_select_preempt: the commit loop holds a job that "
                          "preempted a running job back)"),
    "admit_no_mask_no_admit_step": (0, ""),
    "admit_no_mask_after_a_plain_cycle": (0, ""),
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
    _check(_build(tmp_path, "running_preempt_host_test", []))


def test_the_same_cases_under_address_and_ub_sanitizers(tmp_path):
    """A stand-alone program with its own main: the sanitizer runtime is linked in, nothing is preloaded."""
    exe = _build(tmp_path, "running_preempt_host_test_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    _check(exe)
