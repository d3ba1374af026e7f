"""tests/valid_pyref.py, the truth of the validity check (include/crane_gpu_valid/validity.h), held to the hand-derived table of
tests/valid_case.py — one case per code and the distinctions that matter —, to the existing oracle (a job the oracle places is valid), and
the generator of the GPU tests to its mix of codes (asserted here, so that a GPU test cannot pass on an all-OK batch)."""
import numpy as np
import pytest

from cranesched_amd import abi, synth
from tests import valid_case as vc
from tests import valid_pyref as ref


def test_hand_cases():
    cl, resv, jobs, want_code, want_elig = vc.hand()
    code, elig = ref.check(cl, jobs, ref.resv_node_sets(resv))
    for i, h in enumerate(vc.HAND):
        assert (int(code[i]), int(elig[i])) == (h[2], h[3]), f"case {i} ({h[0]}): got {abi.VALID_STR[int(code[i])]} / {int(elig[i])}"
    assert set(int(c) for c in want_code) == set(range(11)), "the table has a case of every code"


@pytest.mark.parametrize("table", ["one64", "eight_by_8_four_names", "mem_2pow63"])
def test_hand_cases_on_wide_layouts(table):
    """The rows decided by the clamp of a request byte, by a byte's neighbour, by 257-node sums and by the saturated memory sum."""
    cl, jobs, want_code, want_elig, rows = vc.hand_wide()[table]
    code, elig = ref.check(cl, jobs, None)
    for i, r in enumerate(rows):
        assert (int(code[i]), int(elig[i])) == (r[2], r[3]), f"{table} row {i} ({r[0]}): got {abi.VALID_STR[int(code[i])]} / {int(elig[i])}"
    assert {abi.VALID_OK, abi.VALID_NOT_ENOUGH_NODES} <= set(int(c) for c in want_code)
    if table == "one64":
        assert abi.VALID_NO_RESOURCE in want_code and int(cl.gres_slots[0]) >> 63 == 1 and cl.num_nodes == 263
        assert {63, 64, 65, 127, 255} <= set(jobs.gres_total[:, 0].tolist()) and {63, 64, 65, 127, 255} <= set(jobs.gres_spec[:, 0].tolist())
    if table == "eight_by_8_four_names":
        assert jobs.gres_spec.any(axis=0).all() and jobs.gres_total.any(axis=0).all(), "every class index and every name is asked for"


def test_hand_cases_without_reservations():
    """cns_set_reservations is optional: without it every reservation index is unknown."""
    cl, _, jobs, want_code, _ = vc.hand()
    code, _ = ref.check(cl, jobs, None)
    rsv = jobs.reservation != vc.NONE
    later = np.isin(want_code, (abi.VALID_RESV_NODE, abi.VALID_NOT_ENOUGH_NODES, abi.VALID_OK, abi.VALID_RESV_NOT_FOUND))
    assert (code[rsv & later] == abi.VALID_RESV_NOT_FOUND).all() and np.array_equal(code[~rsv], want_code[~rsv])
    assert np.array_equal(code[rsv & ~later], want_code[rsv & ~later])


def test_generator_mix():
    """Over the seeds the GPU tests use: every code in at least 2 % of the jobs, OK in at most 60 %."""
    codes = np.concatenate([vc.generated(s)[3] for s in vc.GPU_SEEDS])
    share = np.bincount(codes, minlength=11) / len(codes)
    for c in range(11):
        assert share[c] >= 0.02, f"{abi.VALID_STR[c]}: {share[c]:.3f} of {len(codes)} jobs"
    assert share[abi.VALID_OK] <= 0.60
    for s in vc.GPU_SEEDS:
        cl, _, jobs, code, elig = vc.generated(s)
        assert cl.num_partitions <= 4 and cl.num_nodes <= 300 and jobs.num_jobs <= 500
        assert (elig[~np.isin(code, (abi.VALID_OK, abi.VALID_NOT_ENOUGH_NODES))] == 0).all()
    some = vc.generated(0)[0]
    assert some.schedulable is not None and not some.schedulable.all() and some.unsupported is not None and some.unsupported.any()
    shared = sum(len(np.unique(vc.generated(s)[0].part_nodes)) < len(vc.generated(s)[0].part_nodes) for s in vc.GPU_SEEDS)
    assert shared >= 10, "most clusters have partitions that share nodes"


def test_generated_snapshots_are_accepted():
    """cns_set_nodes refuses a snapshot whose every partition the cycle refuses, and a partition connected through shared schedulable
    nodes to one that lists an unsupported node is refused with it: every generated cluster keeps a partition outside that, with a
    schedulable node, and stays far below the cycle's 64 distinct res_total records."""
    for s in vc.GPU_SEEDS:
        cl = vc.generated(s)[0]
        lists = [set(int(n) for n in cl.part_nodes[cl.part_offsets[p]:cl.part_offsets[p + 1]]) for p in range(cl.num_partitions)]
        live = [set(n for n in l if cl.schedulable[n]) for l in lists]
        refused = [any(cl.unsupported[n] for n in l) for l in live]
        changed = True
        while changed:                                              # (refusal spreads over shared schedulable nodes to a fixed point)
            changed = False
            for a in range(len(live)):
                for b in range(len(live)):
                    if refused[a] and not refused[b] and live[a] & live[b]:
                        refused[b] = changed = True
        assert any(not r and l for r, l in zip(refused, live)), f"seed {s}: the cycle serves no partition"
        records = set(zip(cl.cpu_total_raw.tolist(), cl.mem_total.tolist(), cl.gres_slots.tolist()))
        assert len(records) <= 16


@pytest.mark.parametrize("name", ["C1", "C2", "C3", "C4"])
def test_placement_implies_validity(built, name):
    """Every job the oracle starts or backfills is valid: code OK with eligible >= node_num."""
    from oracle import pyoracle
    cluster, jobs, now = synth.make_config(name, J=300, N=128, P=4)
    pl = pyoracle.select(cluster, jobs, now).placements
    placed = np.flatnonzero(np.asarray(pl.start_sec[:jobs.num_jobs]) != 0)
    assert len(placed) >= 20, "the configuration places some jobs"
    code, elig = ref.check(cluster, jobs, None)
    bad = [int(j) for j in placed if code[j] != abi.VALID_OK or elig[j] < jobs.node_num[j]]
    assert not bad, f"{name}: placed but not valid: jobs {bad[:10]} codes {[abi.VALID_STR[int(code[j])] for j in bad[:10]]}"
