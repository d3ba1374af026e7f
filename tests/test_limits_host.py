"""The input rules of cns_set_run_limits / cns_upload_limit_jobs (cranesched_amd/csrc/limits_check_host.inc) and the record space, chain
walk and key ranges they share with the submit limits and the usage tables (acct_space_host.inc), no HIP in either, compiled with g++ and
driven by tests/cpp/limits_host_test.cpp: the space by its numbers (one table of 2^32 - 16 records accepted and of 2^32 - 15 refused, counts
whose 64-bit sum wraps), every rule of include/crane_gpu/run_limits.h at its edge, by its message and in the order the call applies them:
a chain of 6 with its levels and a chain of 7, a cycle, a self-parent, a parent of A, CNS_LIM_NONE as user_acct, a skipped job that is not
read, a select_index equal to the cycle's job count.  The same stand-alone program is built a second time with
-fsanitize=address,undefined and run over the same cases.  No GPU involved, nothing loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "limits_host_test.cpp")

RECORDS = (-4, "cns_set_run_limits: more than 2^32 usage records")
CHAIN = (-4, "account chain longer than CNS_LIM_MAX_CHAIN")
CHAIN_CUT = (-4, "account chain longer than CNS_LIM_MAX_CHAIN (or a cycle)")   # given up after 6 accounts that had no level yet
KEYS = "limit job %d: user / user_acct / account / qos / partition out of range"
SELECT = "limit job %d: select_index outside the last cns_select"

WANT = {
    "space_five_tables": (0, "len=6,20,14,35,2 base=0,6,26,40,75 NR=77 ent=77,80,87 ent_len=3,7,2 NE=12"),
    "space_one_qos_alone": (0, "len=0,0,0,0,1 base=0,0,0,0,0 NR=1 ent=1,1,1 ent_len=0,0,1 NE=1"),
    "space_table_of_2_32_minus_16": (0, "len=0,4294967280,0,0,1 base=0,0,4294967280,4294967280,4294967280 NR=4294967281 "
                                        "ent=4294967281,4294967281,4294967281 ent_len=0,0,1 NE=1"),
    "space_table_of_2_32_minus_15": (1, "refused"),
    "space_sum_that_wraps_64_bits": (1, "refused"),
    "valid": (0, "NR=9 levels=0,1"),
    "no_qos": (-1, "cns_set_run_limits: no QoS"),
    "no_qos_array": (-1, "cns_set_run_limits: no QoS"),
    "no_acct_parent": (-1, "cns_set_run_limits: acct_parent missing"),
    "no_part_limits": (-1, "cns_set_run_limits: part_limits missing"),
    "too_many_records": RECORDS,
    "records_sum_at_2_32_minus_16": RECORDS,
    "limit_records_at_2_32_minus_16": RECORDS,
    "records_sum_at_2_32_minus_17": (0, "NR=4294967279 levels=0,1"),
    "records_sum_that_wraps_64_bits": RECORDS,
    "chain_of_6": (0, "NR=17 levels=0,1,2,3,4,5"),
    "chain_of_6_leaf_first": (0, "NR=17 levels=5,4,3,2,1,0"),
    "two_trees_share_levels": (0, "NR=19 levels=3,0,1,2,0,1,4"),
    "chain_of_7": CHAIN,
    "chain_of_7_leaf_first": CHAIN_CUT,
    "chain_cycle_of_two": CHAIN_CUT,
    "chain_self_parent": CHAIN_CUT,
    "parent_of_A": (-1, "acct_parent out of range"),
    "chain_is_refused_before_a_later_parent": CHAIN_CUT,
    "chain_is_refused_before_max_wall": CHAIN_CUT,
    "negative_qos_max_wall": (-1, "negative Qos max_wall"),
    "negative_partition_max_wall": (-1, "negative partition max_wall"),
    "user_part_limit_index": (-1, "partition limit index out of range"),
    "acct_part_limit_index": (-1, "partition limit index out of range"),
    "no_user": (-1, "cns_upload_limit_jobs: missing array"),
    "no_time_limit": (-1, "cns_upload_limit_jobs: missing array"),
    "no_jobs_needs_no_array": (0, "NR=9 levels=0,1"),
    "too_many_jobs": (-4, "more than 2^32-16 jobs"),
    "user_out_of_range": (-1, KEYS % 2),
    "user_acct_out_of_range": (-1, KEYS % 0),
    "user_acct_none": (-1, KEYS % 1),
    "account_out_of_range": (-1, KEYS % 1),
    "qos_out_of_range": (-1, KEYS % 0),
    "partition_out_of_range": (-1, KEYS % 2),
    "valid_skipped_job_is_not_read": (0, "NR=9 levels=0,1"),
    "select_index_at_the_job_count": (-1, SELECT % 1),
    "keys_are_refused_before_select_index": (-1, KEYS % 0),
    "identity_select_past_the_cycle": (-1, SELECT % 2),
    "valid_identity_select": (0, "NR=9 levels=0,1"),
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
    _check(_build(tmp_path, "limits_host_test", []))


def test_the_same_cases_under_address_and_ub_sanitizers(tmp_path):
    """A stand-alone program with its own main: the sanitizer runtime is linked in, nothing is preloaded."""
    exe = _build(tmp_path, "limits_host_test_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    _check(exe)
