"""The host side of a cycle with preemption (cranesched_amd/csrc/preempt_host.inc, no HIP in there) compiled with g++ and driven by
tests/cpp/preempt_host_test.cpp, without a GPU:
  * hand-derived rows: who may preempt, the flattened QoS lists, the buffer plan at its floors, bounds and clamp, the five refusals by
    status and message and their precedence, the two endings that only write the preempting set out, the input rules of
    cns_select_preempt;
  * the running side of cns_select_preempt against tests/running_preempt_pyref.index() on the ledgers of tests/running_case.py, a snapshot
    whose partitions share nodes and one with reservations (the entries ent_job / ent_slot are the routine's input: they come from
    running_preempt_pyref.entry_order on both sides);
  * the fold of the device's (pending job, reference) pairs against the oracle: its per-job lists emitted as pairs, the jobs' pairs
    interleaved by a seeded shuffle that keeps each job's own order, into result arrays of exactly the oracle's sizes.
The same stand-alone program is built a second time with -fsanitize=address,undefined and run over the same inputs (its arrays are exactly
as long as the header says).  Nothing is loaded into Python."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from cranesched_amd import abi
from tests import kat_preempt
from tests import preempt_seams as ps
from tests import running_case as rc
from tests import running_preempt_pyref as rpp
from tests import running_pyref as rp
from tests.test_preempt import OVERLAP_CASES, overlap_preempt_case, random_preempt_case, resv_preempt_case, stale_dip_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "preempt_host_test.cpp")

W = "cns_select_preempt"
NULL = (-1, W + ": null argument")
PENDING = (-1, W + ": missing pending-job array")
RUNNING = (-1, W + ": missing running-job array")
OUTPUT = (-1, W + ": missing output array")
OK = (0, "")
# Every row below is derived by hand from the rules include/crane_gpu/preempt.h and the comments of preempt_host.inc state, not from a run.
WANT = {
    # pd_qos 2, 0, 1, 1, 1 with two QoS of which only 1 has a list: q == num_qos and the empty list may not
    "may_preempt": (0, "00111 any=1 first_two=0"),
    # jobs 2 and 3 may; job_part = 0, 1, 2, none and nothing for job 4
    "parts": (0, "0,0,1,0,"),
    "qos_lists": (0, "off=0,0,1, flat=0,"),
    "qos_lists_empty": (0, "off=0,0,0, flat=0,"),
    # set_in 9, 3, 9 -> ascending, each once; room for one id only: refused
    "plain_ending": (0, "any=0 off=0,0,0, pre= can= set=3,9,"),
    "plain_ending_refused": (-1, "cns_running_select_preempt: preempting_capacity too small"),
    # J 10, R 20, A 30, P 3, S 7, places 12, pools of 101 nodes of 40 B: cand_cap max(4096, min(31, 64 Mi / 3)), out_cap 4 * 30 + 64; pools 3 * 101 * 40 = 12 120 -> 12 128,
    # lists 3 * 4096 * 4 = 49 152 each, the counter's 16 B, 184 pairs of 8 B
    "plan_small": (0, "cand_cap=4096 out_cap=184 pool_nodes=101 pj4=40 pj8=80 ent_gone=30 slot_head=28 rec4=48 rec_gone=12 off_cand=12128 off_chosen=61280 off_cnt=110432 "
                      "off_out=110448 misc=111920 cnt=16"),
    # J 1000, R 5000, P 8: 6001 between 4096 and 8 Mi; pools 8 * 65 536 * 32 B = 16 Mi, lists 8 * 6001 * 4 = 192 032 each
    "plan_between": (0, "cand_cap=6001 out_cap=24064 pool_nodes=65536 pj4=4000 pj8=8000 ent_gone=5000 slot_head=256 rec4=4000 rec_gone=1000 off_cand=16777216 off_chosen=16969248 "
                        "off_cnt=17161280 off_out=17161296 misc=17353808 cnt=16"),
    # J 50 000, R 50 000, P 1024: 100 001 above 64 Mi / 1024 = 65 536; pools 2 GiB, lists 256 Mi each
    "plan_above": (0, "cand_cap=65536 out_cap=400064 pool_nodes=65536 pj4=200000 pj8=400000 ent_gone=60000 slot_head=4096 rec4=280000 rec_gone=70000 off_cand=2147483648 "
                      "off_chosen=2415919104 off_cnt=2684354560 off_out=2684354576 misc=2687555088 cnt=16"),
    # P 32 768: 64 Mi / P = 2048 below the floor of 4096; A, S, places 0 -> one entry, one slot, one record
    "plan_bound_below_the_floor": (0, "cand_cap=4096 out_cap=40064 pool_nodes=1 pj4=20000 pj8=40000 ent_gone=1 slot_head=4 rec4=4 rec_gone=1 off_cand=524288 off_chosen=537395200 "
                                      "off_cnt=1074266112 off_out=1074266128 misc=1074586640 cnt=16"),
    # J 2^26: 4 J + 64 above 2^28; 2^26 - 17: 2^28 - 4, four below it
    "plan_out_cap_clamped": (0, "cand_cap=67108864 out_cap=268435456 pool_nodes=1 pj4=268435456 pj8=536870912 ent_gone=1 slot_head=4 rec4=268435456 rec_gone=67108864 off_cand=16 "
                                "off_chosen=268435472 off_cnt=536870928 off_out=536870944 misc=2684354592 cnt=16"),
    "plan_out_cap_below_the_clamp": (0, "cand_cap=67108848 out_cap=268435452 pool_nodes=1 pj4=268435388 pj8=536870776 ent_gone=1 slot_head=4 rec4=4 rec_gone=1 off_cand=16 "
                                        "off_chosen=268435408 off_cnt=536870800 off_out=536870816 misc=2684354432 cnt=16"),
    "plan_zeros": (0, "cand_cap=4096 out_cap=64 pool_nodes=65536 pj4=4 pj8=8 ent_gone=1 slot_head=4 rec4=4 rec_gone=1 off_cand=0 off_chosen=0 off_cnt=0 off_out=16 misc=528 cnt=16"),
    # pairs (2, 1) (0, 0) (1, 0) (2, P0) (0, 2); rows 0, 1, 2 are jobs 50, 51, 52; the set holds 51 and 40: job 0 cancels 50 and 52, job 1 meets 50 again, job 2's 51 is in the set
    "fold": (0, "off=0,2,3,5, pre=0,2,0,1,P0, can=50,52, set=40,50,51,52,"),
    # ... the ids from the callback (100 + row), asked for the running references only: nothing of them is in the set
    "fold_row_ids": (0, "off=0,2,3,5, pre=0,2,0,1,P0, can=100,102,101, set=40,51,100,101,102,"),
    "fold_row_ids_fail": (-3, "the pick failed"),
    "fold_nothing": (0, "off=0,0,0,0, pre= can= set=40,51,"),
    "refuse_result_buffer": (-4, W + ": more preemptions than the result buffer holds"),
    "refuse_capacity": (-1, W + ": cns_preempt_out::capacity too small"),
    "refuse_cancel_capacity": (-1, W + ": cancel_capacity too small"),
    "refuse_preempting_capacity": (-1, W + ": preempting_capacity too small"),
    "refuse_attrs_name": (-1, "cns_running_select_preempt_attrs: preempting_capacity too small"),
    "first_result_buffer_then_capacity": (-4, W + ": more preemptions than the result buffer holds"),
    "first_capacity_then_cancel": (-1, W + ": cns_preempt_out::capacity too small"),
    "first_cancel_then_preempting": (-1, W + ": cancel_capacity too small"),
    # the caller's set 9, 4, 9, 3 as it came: neither sorted nor refused
    "pass_through_truncates": (0, "off=0,0,0, pre= can= set=9,4,9,"),
    "pass_through": (0, "off=0,0,0, pre= can= set=9,4,9,3,"),
    "pass_through_no_preempt": (0, "off=0,0,0, pre= can= set="),
    # rows 7, 3, 7, 8; entries of rows 1, 0, 2, 0, 2 ending at 500, 600, 700, 50, 60; now 100; the set 7, 5, 7, 3: row 0 carries id 7 (the first row wins), 5 no longer
    # runs; a job's end is that of its last entry, at least now + 1
    "running_side": (0, "pre=1,1,0,0, set_in=7,7,3, off=0,2,3,5,5, ent=1,3,0,2,4, qos=0,1,0,1, qprio=10,20,10,20, start=90,80,70,60, ent_end=101,101,700,101,60, "
                        "rj_end=101,101,101,0, patched=1"),
    "running_side_empty_set": (0, "pre=0,0,0,0, set_in= off=0,2,3,5,5, ent=1,3,0,2,4, qos=0,1,0,1, qprio=10,20,10,20, start=90,80,70,60, ent_end=500,600,700,50,60, "
                                  "rj_end=101,500,101,0, patched=0"),
    "running_side_nothing_runs": (0, "pre=0, set_in= off=0, ent=0, qos=0, qprio=0, start=0, ent_end= rj_end=0, patched=0"),
    "rule_valid": OK, "rule_no_jobs": NULL, "rule_no_out": NULL, "rule_no_pout": NULL,
    "rule_no_nodes": (-5, W + " before cns_set_nodes"),
    "rule_null_before_order": NULL,
    "rule_tables_from_ledger": (-5, W + ": the running tables were built on the device (cns_running_seed / cns_running_advance); hand the running set in with cns_set_running first"),
    "rule_arrays_valid": OK,
    "rule_no_pd_qos": PENDING, "rule_no_pd_qos_priority": PENDING, "rule_no_pd_priority": PENDING,
    "rule_empty_queue_needs_no_pending_array": OK,
    "rule_no_rn_job_id": RUNNING, "rule_no_rn_qos": RUNNING, "rule_no_rn_qos_priority": RUNNING, "rule_no_rn_start": RUNNING,
    "rule_nothing_runs_needs_no_running_array": OK,
    "rule_no_offsets_out": OUTPUT, "rule_no_preempted_out": OUTPUT, "rule_no_cancelled_out": OUTPUT, "rule_no_preempting_out": OUTPUT,
    "rule_pending_before_running_before_output": PENDING,
    "rule_running_before_output": RUNNING,
    "rule_no_qos_offsets_is_no_rule_here": OK,
}


def _build(tmp, name, extra):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp / name)
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", *extra, "-o", exe, SRC], check=True)
    return exe


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("preempt_host"), "preempt_host_test", [])


@pytest.fixture(scope="module")
def sanitised(tmp_path_factory):
    """A stand-alone program with its own main: the sanitizer runtime is linked in, nothing is preloaded."""
    return _build(tmp_path_factory.mktemp("preempt_host_san"), "preempt_host_test_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])


def _run(exe, *args):
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", r.stdout + r.stderr
    return r.stdout.splitlines()


def _hand_rows(exe):
    got = {}
    for line in _run(exe):
        name, rest = line.split(": ", 1)
        status, _, msg = rest.partition(" ")
        got[name] = (int(status), msg)
    assert sorted(got) == sorted(WANT), "every case ran"
    for name, want in WANT.items():
        assert got[name] == want, name


def test_hand_derived_rows(plain):
    _hand_rows(plain)


def test_hand_derived_rows_under_address_and_ub_sanitizers(sanitised):
    _hand_rows(sanitised)


# ---- the running side of cns_select_preempt against tests/running_preempt_pyref.py -------------------------------------------------------
def _row(values):
    return " ".join(str(int(x)) for x in values) + "\n"


def _numbers(line, name):
    head, _, rest = line.partition(" ")
    assert head == name, line
    return [int(x) for x in rest.split(",") if x]


def index_cases():
    """[(tag, ledger, cluster, reservations, now, the preempting ids)]: two ledgers of tests/running_case.py (the set: every third id, one
    of them twice, one id that no longer runs), a snapshot whose partitions share nodes, one with running jobs inside reservations."""
    out = []
    cluster, _, cycles = rc.scenario(3, cycles=3)
    for n in (0, 2):
        led = cycles[n].before
        ids = [r.job_id for r in led.rows]
        out.append((f"running_case cycle {n}", led, cluster, None, cycles[n].now, ids[::3] + [4242, ids[0]]))
    c, _, now, run, pre = overlap_preempt_case(0)
    out.append(("shared nodes", rp.Ledger.from_running(run, pre.rn_job_id), c, None, now, [int(x) for x in pre.preempting]))
    c, _, now, run, rv, pre = resv_preempt_case(0)
    assert (run.reservation != abi.RESV_NONE).any(), "a condition on the inputs: rows on virtual slots"
    out.append(("reservations", rp.Ledger.from_running(run, pre.rn_job_id), c, rv, now, [int(x) for x in pre.preempting] + [4242]))
    return out


def test_running_side_equals_the_python_index(built, plain, sanitised, tmp_path):
    shared = False
    for n, (tag, led, c, resv, now, preempting) in enumerate(index_cases()):
        node_slots, resv_slots = rpp.layout_of(c, resv)
        want = rpp.index(led, node_slots, resv_slots, now, preempting)
        ents = rpp.entry_order(led, node_slots, resv_slots)
        R, A = len(led.rows), len(ents)
        shared = shared or A > sum(len(r.allocs) for r in led.rows)
        assert any(int(i) not in {r.job_id for r in led.rows} for i in preempting) and want["rj_preempting"].any(), (tag, "a condition on the inputs: an id that no longer runs, one that does")
        qos, qprio, start = [r % 3 for r in range(R)], [10 + r % 7 for r in range(R)], [now - 5 * r for r in range(R)]
        path = str(tmp_path / f"index{n}.txt")
        with open(path, "w") as f:
            f.write(f"{now} {R} {A} {len(preempting)}\n")
            f.write(_row(r.job_id for r in led.rows) + _row(qos) + _row(qprio) + _row(start))
            f.write(_row(r for _, r in ents) + _row(led.rows[r].end_sec for _, r in ents) + _row(preempting))
        for exe in (plain, sanitised):
            o = _run(exe, "index", path)
            got = dict(ent_job=[r for _, r in ents], ent_slot=[q for q, _ in ents], rj_preempting=_numbers(o[0], "rj_preempting")[:R], rj_off=_numbers(o[2], "rj_off"),
                       rj_ent=_numbers(o[3], "rj_ent")[:A], ent_end=_numbers(o[7], "ent_end"), rj_end=_numbers(o[8], "rj_end")[:R])
            assert rpp.same_index(got, want) is None, (tag, rpp.same_index(got, want))
            assert set(_numbers(o[1], "set_in")) == set(want["set_in"]), tag
            assert _numbers(o[4], "rj_qos") == qos and _numbers(o[5], "rj_qprio") == qprio and _numbers(o[6], "rj_start") == start, tag
            assert o[9] == f"patched {int(bool(want['rj_preempting'].any()))}", tag
    assert shared, "a condition on the inputs: one allocation is several entries"


# ---- the fold against the oracle -------------------------------------------------------------------------------------------------------
def fold_cases(shape):
    """[(tag, cluster, jobs, now, running, preempt, reservations)]: every seam case but pool_over (the refusal), and the preemption cases of
    tests/test_preempt.py."""
    out = [(f"seam {name}",) + tuple(ps.case(shape, name).inputs) + (None,) for name in ps.CASE_NAMES if name != "pool_over"]
    out += [(f"kat {name}", c, j, kat_preempt.NOW, r, pre, None) for name, c, j, r, pre, _ in kat_preempt.scenarios()]
    for seed in range(60):
        out.append((f"random {seed}",) + random_preempt_case(500 + seed, N=6 + seed % 7, J=50 + seed % 40, P=1 + seed % 2, running=10 + seed % 11) + (None,))
    out += [(f"overlap {seed} {lay}",) + overlap_preempt_case(seed, layout=lay) + (None,) for seed, lay in OVERLAP_CASES]
    for seed in range(8):
        c, j, now, run, rv, pre = resv_preempt_case(seed)
        out.append((f"resv {seed}", c, j, now, run, pre, rv))
    c, j, r, pre = stale_dip_case()
    out.append(("stale dip", c, j, kat_preempt.NOW, r, pre, None))
    return out


def test_fold_equals_the_oracle(built, plain, sanitised, tmp_path):
    from cranesched_amd import engine
    from oracle import pyoracle
    several_jobs = pending_ref = interleaved = 0
    for n, (tag, c, j, now, run, pre, rv) in enumerate(fold_cases(engine.preempt_shape())):
        ref = pyoracle.select(c, j, now, running=run, reservations=rv, preempt=pre).preempt_out
        lists, cancelled, preempting = ref.lists(), ref.cancelled_ids(), ref.preempting_ids()
        several_jobs += sum(1 for x in lists if x) > 1
        pending_ref += any(is_pd for x in lists for is_pd, _ in x)
        # the jobs' pairs interleaved: a seeded shuffle of which job speaks next, each job's own pairs in its order
        turns = np.array([job for job, x in enumerate(lists) for _ in x], np.int64)
        np.random.default_rng(9000 + n).shuffle(turns)
        interleaved += bool(len(turns) and (np.diff(turns) < 0).any())
        at = [0] * len(lists)
        pairs = []
        for job in turns:
            is_pd, x = lists[job][at[job]]
            at[job] += 1
            pairs += [int(job), x | (abi.PREEMPT_REF_PENDING if is_pd else 0)]
        running = {int(x) for x in pre.rn_job_id}
        set_in = [int(x) for x in pre.preempting if int(x) in running]
        path = str(tmp_path / f"fold{n}.txt")
        with open(path, "w") as f:
            cnt = len(turns)
            f.write(f"{j.num_jobs} {len(pre.rn_job_id)} {cnt} {cnt} {cnt} {len(cancelled)} {len(preempting)} {len(set_in)} {n % 2}\n")
            f.write(_row(pre.rn_job_id) + _row(set_in) + _row(pairs))
        offsets = np.cumsum([0] + [len(x) for x in lists])
        flat = [x | (abi.PREEMPT_REF_PENDING if is_pd else 0) for lst in lists for is_pd, x in lst]
        for exe in (plain, sanitised):
            o = _run(exe, "fold", path)
            assert o[0].strip() == "0", (tag, o[0])
            assert _numbers(o[1], "offsets") == [int(x) for x in offsets], tag
            assert [int(x[1:]) | abi.PREEMPT_REF_PENDING if x[0] == "P" else int(x) for x in o[2].partition(" ")[2].split(",") if x] == flat, tag
            assert _numbers(o[3], "cancelled") == cancelled, tag
            assert _numbers(o[4], "preempting") == preempting, tag
    assert several_jobs and pending_ref and interleaved, "conditions on the inputs: preemptions on behalf of several pending jobs, a pending job's reference, pairs that interleave"
