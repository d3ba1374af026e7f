"""The input rules of cns_set_submit_limits / cns_check_submissions (cranesched_amd/csrc/submit_check_host.inc, no HIP in there) compiled
with g++ and driven by tests/cpp/submit_host_test.cpp: every rule of include/crane_gpu_submit/submit_limits.h at its edge, by its message
and in the order the call applies them: records + entities at 2^32 - 17 accepted and at 2^32 - 16 refused, counts whose 64-bit sum wraps,
a chain of 6 accepted and a chain of 7 refused, a cycle, a self-parent, a parent of A, CNS_LIM_NONE as user_acct, a skipped job that is not
read, the largest count + the sum of count at 2^32 - 1 and at 2^32 with and without CNS_SUBMIT_CARRY.  The same stand-alone program is
built a second time with -fsanitize=address,undefined and run over the same cases.  No GPU involved, nothing loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "submit_host_test.cpp")

TABLE = (-1, "cns_set_submit_limits: missing table")
RECORDS = (-4, "cns_set_submit_limits: more than 2^32 - 16 records")
PARENT = (-1, "cns_set_submit_limits: acct_parent out of range")
NO_END = "cns_set_submit_limits: the chain of account %d does not end"
LONG = "cns_set_submit_limits: account %d: a chain of more than 6 accounts"
INDEX = (-1, "cns_set_submit_limits: partition limit index out of range")
KEYS = "cns_check_submissions: job %d: a key index out of range"
SUM = (-4, "cns_check_submissions: the largest submit count + the sum of count over the call exceeds UINT32_MAX")

WANT = {
    "valid": (0, "NR=9 NE=5"),
    "valid_no_accounts_no_tables": (0, "NR=5 NE=3"),
    "no_qos": TABLE,
    "no_acct_parent": TABLE,
    "no_part_limits": TABLE,
    "missing_table_before_gres": TABLE,
    "gres_classes": (-1, "cns_set_submit_limits: gres.num_classes > 8"),
    "gres_class_name": (-1, "cns_set_submit_limits: gres class name id >= 4"),
    "too_many_records": RECORDS,
    "records_and_entities_at_2_32_minus_16": RECORDS,
    "records_and_entities_at_2_32_minus_17": (0, "NR=4294967274 NE=5"),
    "records_sum_that_wraps_64_bits": RECORDS,
    "parent_of_A": PARENT,
    "parents_are_refused_before_chains": PARENT,
    "chain_of_6": (0, "NR=17 NE=9"),
    "chain_of_6_leaf_first": (0, "NR=17 NE=9"),
    "chain_of_7": (-4, LONG % 6),
    "chain_of_7_leaf_first": (-4, LONG % 0),
    "chain_of_7_behind_a_short_one": (-4, LONG % 2),
    "chain_cycle_of_two": (-1, NO_END % 0),
    "chain_self_parent": (-1, NO_END % 1),
    "chain_into_a_cycle_of_eight": (-1, NO_END % 1),
    "chains_are_refused_before_limit_indices": (-1, NO_END % 0),
    "user_part_limit_index": INDEX,
    "acct_part_limit_index": INDEX,
    "jobs_count_of_uint32_max": (-1, "cns_set_submit_limits: a jobs_count of UINT32_MAX"),
    "no_partition": (-1, "cns_check_submissions: missing job array"),
    "no_ntasks": (-1, "cns_check_submissions: missing job array"),
    "valid_no_node_cpu_no_gres": (0, "NR=9 NE=5"),
    "no_user": (-1, "cns_check_submissions: missing key array"),
    "no_count": (-1, "cns_check_submissions: missing key array"),
    "no_code": (-1, "cns_check_submissions: missing result array"),
    "no_time_limit_out": (-1, "cns_check_submissions: missing result array"),
    "user_out_of_range": (-1, KEYS % 2),
    "user_acct_out_of_range": (-1, KEYS % 0),
    "account_out_of_range": (-1, KEYS % 1),
    "qos_out_of_range": (-1, KEYS % 0),
    "partition_out_of_range": (-1, KEYS % 2),
    "valid_skipped_job_is_not_read": (0, "NR=9 NE=5"),
    "keys_are_refused_before_the_sum": (-1, KEYS % 2),
    "sum_at_uint32_max": (0, "NR=9 NE=5"),
    "sum_at_2_32": SUM,
    "sum_of_counts_alone_at_2_32": SUM,
    "carry_sum_at_uint32_max": (0, "NR=9 NE=5"),
    "carry_sum_at_2_32": SUM,
    "without_carry_the_last_call_does_not_count": (0, "NR=9 NE=5"),
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
    _check(_build(tmp_path, "submit_host_test", []))


def test_the_same_cases_under_address_and_ub_sanitizers(tmp_path):
    """A stand-alone program with its own main: the sanitizer runtime is linked in, nothing is preloaded."""
    exe = _build(tmp_path, "submit_host_test_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    _check(exe)
