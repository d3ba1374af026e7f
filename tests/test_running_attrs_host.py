"""The input rules of the calls of include/crane_gpu_running/running_attrs.h (cranesched_amd/csrc/running_attrs_check_host.inc, no HIP in
there) compiled with g++ and driven by tests/cpp/running_attrs_host_test.cpp: every refusal by its status and message — the attribute
arrays of a seed and of a cycle boundary, the state the consumers need, the pending side of cns_priority_order_resident, the arrays
cns_running_select_preempt_attrs must not be handed, and the two refusals that start from a device flag word (the account row, the sum
row; which of three recorded rows decides).  The same stand-alone program is built a second time with -fsanitize=address,undefined and
run over the same cases.  No GPU involved, nothing loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "running_attrs_host_test.cpp")

OK = (0, "")
HINT = "the ledger carries no attribute columns (a plain cns_running_seed / cns_running_advance drops them: seed with cns_running_seed_attrs)"
DROPPED = "(cns_set_running and a changed num_nodes drop the ledger)"
SEED = (-1, "cns_running_seed_attrs: missing attribute array")
STEP = (-1, "cns_running_advance_attrs: missing attribute array of the queue (qos, qos_priority, partition_priority, account)")
ORDER_NULL = (-1, "cns_priority_order_resident: null argument")
ORDER_PENDING = (-1, "cns_priority_order_resident: missing pending array")
CALL = "cns_running_select_preempt_attrs"
CALL_NULL = (-1, CALL + ": null argument")
CALL_RN = (-1, CALL + ": rn_job_id, rn_qos, rn_qos_priority and rn_start_sec must be NULL: the call reads the ledger's columns, not the caller's arrays")
WANT = {
    "seed_valid": OK, "seed_empty_set_needs_no_attrs": OK,
    "seed_no_attrs": SEED, "seed_no_start": SEED, "seed_no_qos": SEED, "seed_no_qos_priority": SEED, "seed_no_partition_priority": SEED, "seed_no_account": SEED,
    "step_valid": OK, "step_start_is_not_read": OK, "step_no_admit_step_needs_no_attrs": OK,
    "step_no_columns": (-5, "cns_running_advance_attrs: " + HINT),
    "step_no_attrs": STEP, "step_no_qos": STEP, "step_no_qos_priority": STEP, "step_no_partition_priority": STEP, "step_no_account": STEP,
    "get_valid": OK, "get_sizes_only": OK,
    "get_null": (-1, "cns_running_get_attrs: null argument"),
    "get_no_ledger": (-5, "cns_running_get_attrs before cns_running_seed_attrs " + DROPPED),
    "get_no_columns": (-5, "cns_running_get_attrs: " + HINT),
    "get_too_small": (-1, "cns_running_get_attrs: the arrays are smaller than the ledger"),
    "order_valid": OK,
    "order_no_cfg": ORDER_NULL, "order_no_pending": ORDER_NULL, "order_no_num_ordered": ORDER_NULL,
    "order_no_order_out": ORDER_PENDING, "order_no_priority_out": ORDER_PENDING, "order_no_submit": ORDER_PENDING, "order_no_pending_account": ORDER_PENDING,
    "order_empty_queue_needs_no_array": OK,
    "order_no_ledger": (-5, "cns_priority_order_resident before cns_running_seed_attrs " + DROPPED),
    "order_no_columns": (-5, "cns_priority_order_resident: " + HINT),
    "order_pending_account": (-1, "pending job account >= num_accounts"),
    "order_pending_negative_cpu": (-1, "negative cpu request"),
    # which recorded row decides: <kind> row=<row>; 1 account, 2 a sum outside its type, 3 a negative cpu sum
    "worst_none": (0, "row=4294967295"), "worst_account_least": (1, "row=2"), "worst_range_least": (2, "row=3"), "worst_negative_least": (3, "row=1"),
    "worst_account_before_range_on_one_row": (1, "row=4"),
    "row_account": (-1, "cns_priority_order_resident: ledger row 5 carries account 64, num_accounts is 64 (running job account >= num_accounts)"),
    "row_negative": (-1, "cns_priority_order_resident: the cpu of ledger row 9's allocations sums to a negative value (negative cpu allocation)"),
    "row_range": (-4, "cns_priority_order_resident: the allocations of ledger row 0 sum to a cpu value outside int64 or a memory value outside uint64"),
    "call_valid": OK,
    "call_no_jobs_arg": CALL_NULL, "call_no_preempt_arg": CALL_NULL, "call_no_out_arg": CALL_NULL, "call_no_pout_arg": CALL_NULL,
    "call_no_nodes": (-5, CALL + " before cns_set_nodes"),
    "call_no_ledger": (-5, CALL + " before cns_running_seed_attrs " + DROPPED),
    "call_no_columns": (-5, CALL + ": " + HINT),
    "call_tables_not_the_ledgers": (-5, CALL + ": the per-slot running tables are not the ledger's (cns_set_nodes / cns_set_reservations emptied them: call "
                                        "cns_running_advance_attrs first)"),
    "call_too_many_pending": (-4, CALL + ": 2^31 pending jobs or more (bit 31 of a reference marks a pending job)"),
    "call_too_many_rows": (-4, CALL + ": 2^31 ledger rows or more (bit 31 of a reference marks a pending job)"),
    "call_rn_job_id_given": CALL_RN, "call_rn_qos_given": CALL_RN, "call_rn_qos_priority_given": CALL_RN, "call_rn_start_given": CALL_RN,
    "call_no_pd_qos": (-1, CALL + ": missing pending-job array"),
    "call_no_qos_offsets": (-1, CALL + ": missing array: the QoS preempt lists"),
    "call_no_set": (-1, CALL + ": missing array: preempting_job_ids"),
    "call_no_offsets_out": (-1, CALL + ": missing output array"),
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
    _check(_build(tmp_path, "running_attrs_host_test", []))


def test_the_same_cases_under_address_and_ub_sanitizers(tmp_path):
    """A stand-alone program with its own main: the sanitizer runtime is linked in, nothing is preloaded."""
    exe = _build(tmp_path, "running_attrs_host_test_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    _check(exe)
