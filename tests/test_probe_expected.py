"""The yardstick of the what-if probes, validated without a GPU: tests/probe_case.expected (one oracle cycle per probe over
`ordered jobs + [probe]`, result of the last job) gives the same answers with the restated oracle and with the reference's own compiled
NodeSelect (oracle/_ref) — the definition of a probe's answer is pinned to the reference.  Also asserted here, on the oracle's answers:
the outcome mix tests/test_gpu_probe.py relies on, so that the GPU file cannot pass by asking only easy questions."""
import numpy as np
import pytest

from cranesched_amd import abi
from oracle import pyoracle
from tests import probe_case as pc


def _both(c, j, p, now, run, rv=None, batch=0):
    exp = pc.expected(c, j, p, now, running=run, reservations=rv, batch=batch, backend="oracle")
    if pyoracle.ref_available():
        ref = pc.expected(c, j, p, now, running=run, reservations=rv, batch=batch, backend="ref")
        assert exp.diff(ref) is None, f"oracle and reference disagree on a probe: {exp.diff(ref)}"
    return exp


def test_concat_and_take_keep_every_field(built):
    from tests import helpers
    j = helpers.random_case(3, J=50)[1]
    a, b = pc.take(j, np.arange(20)), pc.take(j, np.arange(20, 50))
    ab = pc.concat(a, b)
    for f in ("partition", "time_limit_sec", "node_mem", "task_cpu_raw", "task_mem", "node_num", "ntasks", "ntasks_per_node_min",
              "ntasks_per_node_max", "exclusive", "gres_total", "gres_spec", "skip", "incl_offsets", "excl_offsets"):
        assert np.array_equal(getattr(ab, f), getattr(j, f)), f
    assert np.array_equal(ab.incl_nodes[:int(ab.incl_offsets[-1])], j.incl_nodes[:int(j.incl_offsets[-1])])
    assert np.array_equal(ab.excl_nodes[:int(ab.excl_offsets[-1])], j.excl_nodes[:int(j.excl_offsets[-1])])
    plain = abi.Jobs(partition=[0], time_limit_sec=[60], node_mem=[0], task_cpu_raw=[256], task_mem=[1], node_num=[1], ntasks=[1],
                     ntasks_per_node_min=[1], ntasks_per_node_max=[1])
    m = pc.concat(j, plain)     # a side without the optional arrays
    assert m.num_jobs == 51 and m.skip[-1] == 0 and m.exclusive[-1] == 0 and not m.gres_total[-1].any()
    assert m.incl_offsets[-1] == m.incl_offsets[-2] and m.excl_offsets[-1] == m.excl_offsets[-2]


def test_expected_is_the_last_job_of_the_extended_queue(built):
    """A probe that IS the next job of the queue: its expected answer is what the full cycle writes for that job."""
    from tests import helpers
    c, j, now, run = helpers.random_case(2, J=300)
    full = pyoracle.select(c, j, now, running=run).placements
    for cut in (120, 250, 299):
        exp = pc.expected(c, pc.take(j, np.arange(cut)), pc.take(j, [cut]), now, running=run)
        assert exp.start_sec[0] == full.start_sec[cut] and exp.reason[0] == full.reason[cut]
        a, b = int(full.place_offsets[cut]), int(full.place_offsets[cut + 1])
        assert np.array_equal(exp.node_idx[:b - a], full.node_idx[a:b]) and np.array_equal(exp.cpu_raw[:b - a], full.cpu_raw[a:b])


def test_random_scenarios_oracle_equals_reference_and_cover_every_outcome(built):
    mix = {}
    for seed in pc.RANDOM_SEEDS:
        c, j, p, now, run = pc.random_scenario(seed)
        exp = _both(c, j, p, now, run)
        mix = pc.add_mix(mix, pc.outcome_mix(exp, p, now))
    print("outcome mix over the random scenarios:", mix)
    pc.check_mix(mix)


def test_reservation_scenario_oracle_equals_reference(built):
    c, j, p, now, run, rv = pc.resv_scenario(0)
    exp = _both(c, j, p, now, run, rv)
    r = exp.reason[:p.num_jobs]
    assert (r == abi.REASON_RESERVATION_NOT_FOUND).sum() > 0, "probes into an unknown / inactive reservation"
    assert ((r == abi.REASON_NONE) | (r == abi.REASON_PRIORITY) | (r == abi.REASON_RESOURCE)).sum() > 10


def test_shared_node_scenario_oracle_equals_reference(built):
    c, j, p, now, run = pc.overlap_scenario(1)
    exp = _both(c, j, p, now, run)
    m = pc.outcome_mix(exp, p, now)
    assert m["now"] > 0 and m["later"] > 0, m


def test_batch_limit_scenario_oracle_equals_reference(built):
    c, j, p, now, run = pc.random_scenario(1)
    exp = _both(c, j, p, now, run, batch=j.num_jobs // 2)
    full = pc.expected(c, j, p, now, running=run)
    assert exp.diff(full) is not None, "the state after half of the queue must answer some probe differently"


def test_hand_made_resource_reserved_probe(built):
    c, j, p, now, run, rv, (start, reason) = pc.reserved_kat()
    exp = _both(c, j, p, now, run, rv)
    assert (int(exp.start_sec[0]), int(exp.reason[0])) == (start, reason)
    assert exp.node_idx[0] == 0 and exp.cpu_raw[0] == 4 * 256
