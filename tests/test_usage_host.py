"""The input rules of cns_usage_set_tables / cns_usage_apply (cranesched_amd/csrc/usage_check_host.inc, no HIP in there) compiled with g++
and driven by tests/cpp/usage_host_test.cpp: every rule of include/crane_gpu_usage/usage.h at its edge, by its message: a chain of 6
accepted and a chain of 7 refused, a cycle in acct_parent, 2^24 + 1 rows (by the count alone; at 2^24 the pass reaches the arrays), the
all-zero row, negative values, CNS_LIM_NONE as user_acct in a release and in a charge, a skipped row that is not read.  The same
stand-alone program is built a second time with -fsanitize=address,undefined and run over the same cases.  No GPU involved, nothing
loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "usage_host_test.cpp")

WANT = {
    "valid": (0, "NR=50 NE=11 applied=3"),
    "valid_skipped_row_is_not_read": (0, "NR=50 NE=11 applied=2"),
    "valid_only_keys_and_one_delta": (0, "NR=50 NE=11 applied=3"),
    "valid_class_count_alone": (0, "NR=50 NE=11 applied=3"),
    "valid_charge": (0, "NR=50 NE=11 applied=3"),
    "chain_of_7": (-4, "cns_usage_set_tables: account 6: a chain of more than 6 accounts"),
    "chain_cycle": (-1, "cns_usage_set_tables: the chain of account 0 does not end"),
    "chain_self": (-1, "cns_usage_set_tables: the chain of account 6 does not end"),
    "parent_out_of_range": (-1, "cns_usage_set_tables: acct_parent[3] out of range"),
    "no_parent": (-1, "cns_usage_set_tables: missing array: acct_parent"),
    "gres_classes": (-1, "cns_usage_set_tables: gres.num_classes > 8"),
    "gres_class_name": (-1, "cns_usage_set_tables: gres class name id >= 4"),
    "table_negative_cpu": (-1, "cns_usage_set_tables: a negative cpu_raw or wall_sec in table 0"),
    "table_negative_wall": (-1, "cns_usage_set_tables: a negative cpu_raw or wall_sec in table 4"),
    "too_many_records": (-4, "cns_usage_set_tables: more than 2^32 - 16 records"),
    "too_many_jobs": (-4, "cns_usage_apply: more than 2^24 jobs in one call"),
    "jobs_at_the_limit_reach_the_arrays": (-1, "cns_usage_apply: missing key array"),
    "unknown_op": (-1, "cns_usage_apply: unknown op"),
    "no_user": (-1, "cns_usage_apply: missing key array"),
    "no_user_acct": (-1, "cns_usage_apply: missing key array"),
    "no_account": (-1, "cns_usage_apply: missing key array"),
    "no_qos": (-1, "cns_usage_apply: missing key array"),
    "no_partition": (-1, "cns_usage_apply: missing key array"),
    "no_not_found": (-1, "cns_usage_apply: missing result array"),
    "no_over_free": (-1, "cns_usage_apply: missing result array"),
    "user_out_of_range": (-1, "cns_usage_apply: job 2: a key index out of range"),
    "user_acct_out_of_range": (-1, "cns_usage_apply: job 0: a key index out of range"),
    "account_out_of_range": (-1, "cns_usage_apply: job 1: a key index out of range"),
    "qos_out_of_range": (-1, "cns_usage_apply: job 0: a key index out of range"),
    "partition_out_of_range": (-1, "cns_usage_apply: job 1: a key index out of range"),
    "negative_cpu": (-1, "cns_usage_apply: job 0: a negative cpu_raw or wall_sec"),
    "negative_wall": (-1, "cns_usage_apply: job 2: a negative cpu_raw or wall_sec"),
    "all_zero_row": (-1, "cns_usage_apply: job 1: a delta that is all zero"),
    "charge_without_user_acct": (-1, "cns_usage_apply: job 1: a charge without a user_acct"),
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
    _check(_build(tmp_path, "usage_host_test", []))


def test_the_same_cases_under_address_and_ub_sanitizers(tmp_path):
    """A stand-alone program with its own main: the sanitizer runtime is linked in, nothing is preloaded."""
    exe = _build(tmp_path, "usage_host_test_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    _check(exe)
