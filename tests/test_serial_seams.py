"""The seam cases of the serial protocol (tests/serial_seams.py) on the CPU: every case's CONDITION — what puts it on its seam, the place
of every needle in the scanners' and the helpers' loops included — holds on the oracle's own answers, the reference build (where there
is one) places every job as the oracle does, the generators are deterministic, the case list covers every field of cns_serial_shape,
pad() changes no answer of the case it pads, and the rule busy partitions -> helper count | k_mem is the launch plan's own
(csrc/plan_host.inc through tests/cpp/plan_host_test.cpp).  tests/test_gpu_serial_seams.py holds the engine to the oracle on the same cases."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import select_seams as ss
from tests import serial_seams as sr
from tests.test_select_seams import NO_NODE_FITS, same_arrays

SHAPE = sr.SHIPPED
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HAND = ("N", "H", "W", "G", "P")


def oracle_runner(case, backend="oracle"):
    """ora(n): the oracle's run of the first n jobs of the case's queue (None: all of it), each computed once."""
    from oracle import pyoracle
    memo = {}

    def ora(n=None):
        if n not in memo:
            specs = case.specs if n is None else (case.specs[:n] or NO_NODE_FITS)
            memo[n] = pyoracle.select(case.cluster, sr.jobs_of(specs), case.now, running=case.running, backend=backend, **case.cfg)
        return memo[n]
    return ora


def same_case(case, rebuilt):
    assert same_arrays(case.cluster, rebuilt.cluster) and same_arrays(case.jobs, rebuilt.jobs) and case.specs == rebuilt.specs and case.cfg == rebuilt.cfg
    assert (case.running is None) == (rebuilt.running is None) and (case.running is None or same_arrays(case.running, rebuilt.running))
    assert case.nodes == rebuilt.nodes and case.covers == rebuilt.covers and case.kernel == rebuilt.kernel and (case.busy, case.whole) == (rebuilt.busy, rebuilt.whole)
    return True


def groups_of(cluster):
    """partition -> its group: the partitions that share a node are one scheduler of the engine (one busy partition of the launch plan)."""
    off, pn = cluster.part_offsets, cluster.part_nodes
    group, owner = list(range(cluster.num_partitions)), {}
    find = lambda p: p if group[p] == p else find(group[p])
    for p in range(cluster.num_partitions):
        for n in np.unique(pn[int(off[p]):int(off[p + 1])]).tolist():
            q = owner.setdefault(n, p)
            if find(q) != find(p):
                group[find(p)] = find(q)
    return [find(p) for p in range(cluster.num_partitions)]


def check_case(case, ref_too=True):
    from oracle import pyoracle
    ora = oracle_runner(case)
    seen = case.condition(ora)
    assert isinstance(seen, dict) and seen
    with_jobs = {int(p) for p in case.jobs.partition}
    busy = len({groups_of(case.cluster)[p] for p in with_jobs})
    assert busy == case.busy and case.whole == (len(with_jobs) == case.cluster.num_partitions), (case.name, busy)
    assert case.kernel[0] != "giant" or case.kernel[1] == sr.plan_rule(SHAPE, busy), (case.name, case.kernel)
    if ref_too and pyoracle.ref_available() and not case.cfg:   # (as tests/test_select_seams.py: the reference's limits are compile-time constants)
        ref = oracle_runner(case, backend="ref")()
        assert ref.placements.diff(ora().placements) is None, case.name
        for n in case.nodes[:4]:
            a, b = ref.timeline(int(n)), ora().timeline(int(n))
            assert all(np.array_equal(a[f], b[f]) for f in a), (case.name, n)
    return seen


def test_the_case_lists_are_built_for_the_shape_the_library_exports(built):
    from cranesched_amd import engine
    assert engine.serial_shape() == SHAPE and engine.select_shape() == ss.SHIPPED


def test_the_case_names_cover_every_field_of_the_shape():
    covered, names = set(), []
    for fam in HAND + ("Q",) + sr.R_FAMILIES:
        for c in sr.cases(SHAPE, fam).values():
            covered |= set(c.covers)
            names.append((fam, c.name))
    assert covered == set(SHAPE._fields), set(SHAPE._fields) ^ covered
    L, T, HL, HT, nh = SHAPE.scan_lanes, SHAPE.scan_trip_rows, SHAPE.helper_lanes, SHAPE.helper_trip_slots, SHAPE.helpers_min
    n_names = sr.case_names(SHAPE, "N")
    for tag in ("L-1", "L", "L+1", "TL-1", "TL", "TL+1", "64L-1", "64L", "64L+1"):
        assert all(f"{kind}_{tag}_{inst}" in n_names for kind in ("one", "pair", "phantom") for inst in ("giant", "mem")), tag
    widest = max(c.cluster.num_nodes for c in sr.cases(SHAPE, "N").values())
    assert widest <= 64 * L + 1 + T * L + 16, "no case of family N wider than the second mask word plus one trip (and the pads)"
    h = sr.cases(SHAPE, "H")
    sizes = {c.cluster.num_nodes - (c.busy - 1) for c in h.values()}
    assert {HL * nh - 1, HL * nh + 1, HT * HL * nh - 1, HT * HL * nh + 1, HL * 64 - 1, HL * 64 + 1} <= sizes and min(sizes) < HL
    assert {c.kernel[1][1] for c in h.values()} == {4, 9, 12, 21, 64}
    assert {n.rsplit("_", 1)[0] for n in sr.case_names(SHAPE, "W")} == {"window", "ntasks", "exclusive", "phase_b", "lists"}
    assert all(c.cluster.num_nodes - (c.busy - 1) == 64 * L + 1 for c in sr.cases(SHAPE, "W").values())
    for f in sr.REPLAYED:
        assert [c.name for c in sr.cases(SHAPE, "R" + f).values()] == ss.case_names(ss.SHIPPED, f)
        assert [c.name for c in sr.cases(SHAPE, f"R{f}_pad").values()] == [n + "_pad16" for n in ss.case_names(ss.SHIPPED, f)]
    other = SHAPE._replace(scan_lanes=64, scan_trip_rows=2, helper_lanes=128, helpers_min=8)
    assert {"one_TL+1_mem", "pair_64L_giant"} <= set(sr.case_names(other, "N")) and max(c.cluster.num_nodes for c in sr.cases(other, "N").values()) == 64 * 64 + 1 + 8


@pytest.mark.parametrize("family,name", [(f, n) for f in HAND for n in sr.case_names(SHAPE, f)])
def test_case_meets_its_condition(built, family, name):
    check_case(sr.case(SHAPE, family, name))


def test_the_chain_meets_its_condition(built):
    q = sr.case(SHAPE, "Q", "three_cycles")
    seen = q.condition(oracle_runner)
    assert len(seen["links"]) == 3
    a, b, c = q.chain
    assert same_arrays(a.cluster, b.cluster) and same_arrays(a.running, b.running) and b.jobs.num_jobs < a.jobs.num_jobs, "the second link: the same snapshot, a shorter queue"
    assert c.cluster.num_nodes != a.cluster.num_nodes and len({x.busy for x in q.chain}) == 3


@pytest.mark.parametrize("family", sr.R_FAMILIES)
def test_replayed_select_cases_meet_their_conditions(built, family):
    """Unpadded, a replayed case IS the select case (tests/test_select_seams.py checks those): only its kernel is new.  Padded, its
    condition must hold on the oracle's run of the padded case, and no answer of its own jobs may differ from the unpadded run's."""
    from oracle import pyoracle
    padded = family.endswith("_pad")
    base = ss.cases(ss.SHIPPED, family[1])
    for c in sr.cases(SHAPE, family).values():
        assert c.kernel == ("giant", sr.plan_rule(SHAPE, c.busy)) and c.kernel[1][0] == ("k_mem" if padded else "k_giant")
        if not padded:
            b = base[c.name]
            assert c.cluster is b.cluster and c.jobs is b.jobs and c.running is b.running and c.condition is b.condition and c.nodes == b.nodes
            continue
        b = base[c.name[:-len("_pad16")]]
        check_case(c, ref_too=False)
        own = pyoracle.select(b.cluster, b.jobs, b.now, running=b.running, **b.cfg)
        got = pyoracle.select(c.cluster, c.jobs, c.now, running=c.running, **c.cfg)
        J, K = b.jobs.num_jobs, b.jobs.total_places()
        for f in ("start_sec", "reason"):
            assert np.array_equal(getattr(got.placements, f)[:J], getattr(own.placements, f)[:J]), (c.name, f)
        for f in ("node_idx", "ntasks", "cpu_raw", "mem", "core_lo", "core_hi", "gres", "core_w2", "core_w3"):
            assert np.array_equal(getattr(got.placements, f)[:K], getattr(own.placements, f)[:K]), (c.name, f)
        assert np.array_equal(got.costs()[:len(own.costs())].view(np.uint64), own.costs().view(np.uint64)), c.name


def test_pad_changes_no_answer_of_a_needle_case(built):
    from oracle import pyoracle
    inner = sr.needle_case(SHAPE, "x", 900, free=[3, 899], costly={500: 10}, specs=[sr.one(), sr.one(k=2), sr.one(), sr.one()])
    p = sr.pad(inner, 5)
    assert p.busy == 6 and p.cluster.num_partitions == 6 and p.cluster.num_nodes == 905 and p.jobs.num_jobs == 9
    a = pyoracle.select(inner.cluster, inner.jobs, inner.now, running=inner.running)
    b = pyoracle.select(p.cluster, p.jobs, p.now, running=p.running)
    assert [sr.placed(a.placements, inner.specs, j) for j in range(4)] == [sr.placed(b.placements, p.specs, j) for j in range(4)]
    assert np.array_equal(a.costs().view(np.uint64), b.costs()[:900].view(np.uint64))


@pytest.mark.parametrize("family", HAND + ("Q",))
def test_the_generators_are_deterministic(family):
    kept = sr.cases(SHAPE, family)
    fresh = {c.name: c for c in sr.FAMILIES[family](SHAPE)}
    assert list(kept) == list(fresh)
    for n in kept:
        links = zip(kept[n].chain, fresh[n].chain) if kept[n].chain else [(kept[n], fresh[n])]
        assert all(same_case(a, b) for a, b in links)


def test_the_plan_rule_is_the_launch_plans(tmp_path):
    """sr.plan_rule against plan_serial_launch itself: tests/cpp/plan_host_test.cpp prints what `giant` launches for 1 .. 20 busy partitions."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "plan_host_test")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "plan_host_test.cpp")], check=True)
    out = subprocess.run([exe, "serial", "20"], capture_output=True, text=True, timeout=60, check=True).stdout.split("\n")
    assert out[0] == f"helpers_min {SHAPE.helpers_min}"
    rows = [r.split() for r in out[1:] if r]
    assert [int(r[0]) for r in rows] == list(range(1, 21))
    for busy, kern, nh, giant_masks in rows:
        assert sr.plan_rule(SHAPE, int(busy)) == (kern, int(nh) if kern == "k_giant" else None), (busy, kern, nh)
        assert (giant_masks == "1") == (kern == "k_giant"), "k_mem for partitions of this size: the ordinary masks"
    assert [int(r[2]) for r in rows[:8]] == [64, 32, 21, 16, 12, 10, 9, 8] and rows[15][1:3] == ["k_giant", "4"] and rows[16][1] == "k_mem"
    used = {c.busy for f in HAND for c in sr.cases(SHAPE, f).values()} | {c.busy for c in sr.case(SHAPE, "Q", "three_cycles").chain}
    assert used <= set(range(1, 21)) and {1, 2, 3, 5, 7, 16, 17} <= used
