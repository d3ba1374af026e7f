"""CPU side of the wide-GRES cases (tests/gres_wide.py): the cases provably reach the edges they are for (coverage from the oracle's own
placements), both oracle algebras agree on them (selection, preemption, steps), and the reference's own code agrees with the oracle
at these layouts (feasible on random requests, whole cycles) — so that the GPU tests of tests/test_gpu_gres_wide.py compare the
engine with a pinned oracle."""
import functools

import numpy as np
import pytest

from cranesched_amd import abi
from oracle import pyoracle
from tests import gres_wide as gw

RANDOM = list(range(8))
EDGE_COUNTS = {14, 15, 16, 17, 64, 65, 127, 128, 255}


# ---------------------------------------------------------------------------------------------------------------------------------
# the generator
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lay", gw.NAMED + RANDOM)
def test_layouts_are_valid(lay):
    L = gw.make_layout(lay)
    C = len(L.class_name)
    assert 1 <= C <= abi.MAX_GRES_CLASSES and all(0 <= a < abi.MAX_GRES_NAMES for a in L.class_name)
    assert all(1 <= w <= 64 and s + w <= 64 for s, w in zip(L.class_shift, L.class_width))
    seen = 0
    for m in gw.class_masks(L):
        assert seen & m == 0, "classes overlap"
        seen |= m


def test_named_layouts_reach_the_limits():
    one, eight, un = (gw.make_layout(n) for n in ("one64", "eight_by_8_four_names", "uneven"))
    assert one.class_width == [64] and gw.class_masks(one)[0] == gw.M64
    assert len(eight.class_name) == 8 and sorted(eight.class_name) == [0, 0, 1, 1, 2, 2, 3, 3]
    assert eight.class_shift != sorted(eight.class_shift), "class index and bit position must disagree"
    assert max(s + w for s, w in zip(un.class_shift, un.class_width)) == 64
    per_name = {a: un.class_name.count(a) for a in set(un.class_name)}
    assert 1 in per_name.values() and max(per_name.values()) >= 3     # the fixed-split acnt path and dyn_gres
    assert any(w >= 16 for w in un.class_width)
    # the random family: 1..8 classes, 1..4 names, widths up to 64 among them
    rs = [gw.make_layout(s) for s in range(64)]
    assert {len(r.class_name) for r in rs} >= {1, 8} and {len(set(r.class_name)) for r in rs} >= {1, 4}
    assert max(max(r.class_width) for r in rs) >= 32


def test_exactly_64_types():
    for lay in ("uneven", "eight_by_8_four_names"):
        c, j, now, run = gw.gres_wide_case(80, N=160, J=900, P=2, running=60, layout=lay, types=64)
        assert gw.num_types(c) == abi.MAX_NODE_TYPES
    for lay in gw.NAMED + RANDOM:
        for seed in range(2):
            assert gw.num_types(gw.gres_wide_case(seed, layout=lay)[0]) <= abi.MAX_NODE_TYPES


@pytest.mark.parametrize("lay", gw.NAMED)
def test_requests_cover_the_edges(lay):
    """Typed and untyped counts of 14..17, the class width and one more, 64, 65 and the bytes 127 / 128 / 255; totals equal to and
    above the typed sum; requests on every name of the layout."""
    L = gw.make_layout(lay)
    tot, spec, names = set(), set(), set()
    equal = above = below = multi = 0
    for seed in range(2):
        _, j, _, _ = gw.gres_wide_case(seed, layout=lay)
        gt, gs = j.gres_total.astype(np.int64), j.gres_spec.astype(np.int64)
        tot |= set(gt.ravel().tolist()); spec |= set(gs.ravel().tolist())
        names |= set(np.nonzero(gt.any(axis=0))[0].tolist())
        for x in range(j.num_jobs):
            for a in range(abi.MAX_GRES_NAMES):
                s = sum(int(gs[x, c]) for c in range(len(L.class_name)) if L.class_name[c] == a)
                if s and gt[x, a] == s: equal += 1
                if s and gt[x, a] > s: above += 1
                if s and gt[x, a] < s: below += 1
            multi += int((gt[x] > 0).sum() > 1)
    assert EDGE_COUNTS <= tot and EDGE_COUNTS <= spec
    assert {w for w in L.class_width if w > 1} <= spec and {w + 1 for w in L.class_width} <= spec
    assert names == set(L.class_name)
    assert equal and above and below and (multi or len(names) == 1)


@pytest.mark.parametrize("lay", gw.NAMED)
def test_cases_reach_the_saturation_edges(lay):
    """From the oracle's own placements: start-now placements take >= 16 slots of one class, bit 63 is allocated, every name is allocated,
    exclusive jobs start on nodes with a class of >= 16 slots, jobs are backfilled and impossible requests are refused."""
    L = gw.make_layout(lay)
    tot = dict(max_class_now=0, bit63=False, names=set(), excl_big_now=0, backfilled=0, resource=0)
    for seed in range(2):
        c, j, now, run = gw.gres_wide_case(seed, layout=lay)
        cov = gw.coverage(c, j, pyoracle.select(c, j, now, running=run).placements)
        tot["max_class_now"] = max(tot["max_class_now"], cov["max_class_now"])
        for k in ("excl_big_now", "backfilled", "resource"):
            tot[k] += cov[k]
        tot["bit63"] |= cov["bit63"]; tot["names"] |= cov["names"]
    assert tot["bit63"] and tot["names"] == set(L.class_name)
    assert tot["backfilled"] > 100 and tot["resource"] > 50
    if max(L.class_width) >= 16:
        assert tot["max_class_now"] >= 16 and tot["excl_big_now"] > 0
    if lay == "one64":
        assert tot["max_class_now"] >= 48


def test_running_jobs_hold_big_class_slots():
    """The running allocations take many slots of one class (16 and more on one64), and on some node a class has fewer than 16 free slots
    now and 16 or more once its running jobs end: the front counts cross the 15 / 16 boundary during the cycle."""
    for lay in ("one64", "uneven"):
        c, j, now, run = gw.gres_wide_case(0, layout=lay)
        assert max(max(gw.class_counts(c.gres, int(g))) for g in run.alloc_gres) >= (16 if lay == "one64" else 8)
        free = {int(n): int(c.gres_slots[n]) for n in run.alloc_node}
        for n, g in zip(run.alloc_node, run.alloc_gres):
            free[int(n)] &= ~int(g)
        assert any(f < 16 <= t for n, fm in free.items()
                   for f, t in zip(gw.class_counts(c.gres, fm), gw.class_counts(c.gres, int(c.gres_slots[n]))))


# ---------------------------------------------------------------------------------------------------------------------------------
# the two oracle algebras (literal containers of the reference's types vs masks) agree
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lay", gw.NAMED + RANDOM)
@pytest.mark.parametrize("seed", [0, 1])
def test_selection_mask_vs_literal(lay, seed):
    c, j, now, run = gw.gres_wide_case(seed, layout=lay)
    a = pyoracle.select(c, j, now, running=run)
    b = pyoracle.select(c, j, now, running=run, algebra=pyoracle.LITERAL)
    assert a.placements.diff(b.placements) is None
    assert np.array_equal(a.costs().view(np.uint64), b.costs().view(np.uint64))


@pytest.mark.parametrize("lay", gw.NAMED)
def test_selection_mask_vs_literal_shared_nodes_and_reservations(lay):
    c, j, now, run = gw.gres_wide_case(40, N=64, J=500, P=4, running=30, layout=lay)
    c, j = gw.repartition(c, j, 40, "all+subsets")
    a = pyoracle.select(c, j, now, running=run)
    b = pyoracle.select(c, j, now, running=run, algebra=pyoracle.LITERAL)
    assert a.placements.diff(b.placements) is None
    c, j, now, run, rv = gw.resv_case(50, layout=lay)
    a = pyoracle.select(c, j, now, running=run, reservations=rv)
    b = pyoracle.select(c, j, now, running=run, reservations=rv, algebra=pyoracle.LITERAL)
    assert a.placements.diff(b.placements) is None
    r = a.placements.reason[:j.num_jobs]
    assert (r == abi.REASON_RESOURCE_RESERVED).sum() > 0 and (r == abi.REASON_RESERVATION_NOT_FOUND).sum() > 0


@pytest.mark.parametrize("lay", gw.NAMED)
@pytest.mark.parametrize("seed", [60, 61])
def test_preemption_mask_vs_literal(lay, seed):
    c, j, now, run, pre = gw.preempt_case(seed, N=24, J=400, P=2, running=120, layout=lay)
    a = pyoracle.select(c, j, now, running=run, preempt=pre)
    b = pyoracle.select(c, j, now, running=run, preempt=pre, algebra=pyoracle.LITERAL)
    assert a.placements.diff(b.placements) is None
    assert a.preempt_out.lists() == b.preempt_out.lists()
    assert sum(len(x) for x in a.preempt_out.lists()) > 0


@pytest.mark.parametrize("lay", gw.NAMED + [3, 5])
def test_steps_mask_vs_literal(lay):
    L, jobs, steps = gw.step_case(7, layout=lay, J=600)
    a = pyoracle.schedule_steps(L, jobs, steps, pyoracle.MASK)
    b = pyoracle.schedule_steps(L, jobs, steps, pyoracle.LITERAL)
    assert a.diff(b) is None
    S = steps.num_steps
    assert 0 < a.scheduled[:S].sum() < S


# ---------------------------------------------------------------------------------------------------------------------------------
# the oracle against the reference's own code (oracle/_ref) at these layouts
# ---------------------------------------------------------------------------------------------------------------------------------
ref = pytest.mark.skipif(not pyoracle.ref_available(), reason="oracle/_ref is not built and /root/reference is absent")


def _rand_req(rng, L):
    C, names = len(L.class_name), sorted(set(L.class_name))
    gtot, gspec = [0] * abi.MAX_GRES_NAMES, [0] * abi.MAX_GRES_CLASSES
    pick = lambda w: int(rng.choice([1, 2, 3, 7, 8, 14, 15, 16, 17, w - 1 if w > 1 else 1, w, w + 1, 63, 64, 65, 127, 128, 255]))
    for _ in range(int(rng.integers(1, 4))):
        c = int(rng.integers(0, C)); a = L.class_name[c]
        s = int(rng.integers(0, 4))
        if s == 0: gtot[a] = min(255, pick(sum(L.class_width[x] for x in range(C) if L.class_name[x] == a)))
        elif s == 1: gspec[c] = pick(L.class_width[c]); gtot[a] = max(gtot[a], gspec[c])
        elif s == 2: gspec[c] = pick(L.class_width[c]); gtot[a] = min(255, gspec[c] + int(rng.integers(1, 20)))
        else: gspec[c] = pick(L.class_width[c])
    return gtot, gspec


@ref
@pytest.mark.parametrize("lay", gw.NAMED + RANDOM)
def test_feasible_against_the_reference_code(lay):
    L = gw.make_layout(lay)
    rng = np.random.default_rng(4000 + (lay if isinstance(lay, int) else gw.NAMED.index(lay) + 100))
    cm = gw.class_masks(L)
    full = 0
    for m in cm:
        full |= m
    ok = 0
    for _ in range(3000):
        style = int(rng.integers(0, 3))
        if style == 0: g = full
        elif style == 1: g = full & (int(rng.integers(0, 1 << 62)) | (int(rng.integers(0, 4)) << 62))
        else: g = full & (int(rng.integers(0, 1 << 62)) | int(rng.integers(0, 1 << 62)) | (int(rng.integers(0, 4)) << 62))
        a = pyoracle.make_res(64 * 256, 256 << 30, gw.M64, 0, g)
        gtot, gspec = _rand_req(rng, L)
        req = pyoracle.make_req(int(rng.choice([256, 1024, 128])), int(rng.integers(0, 8)) << 30, gtot, gspec)
        want = pyoracle.feasible(L, 0, req, a, backend="ref")
        for alg in (pyoracle.MASK, pyoracle.LITERAL):
            assert pyoracle.feasible(L, alg, req, a) == want, (lay, gtot, gspec, hex(g))
        ok += want[0]
    assert 200 < ok < 2800, "the requests must both fit and fail"


@ref
@pytest.mark.parametrize("lay", gw.NAMED + [3, 5])
def test_selection_against_the_reference_code(lay):
    from tests.test_ref_pin import both
    c, j, now, run = gw.gres_wide_case(90, N=24, J=200, P=2, running=20, layout=lay)
    both(f"wide GRES {lay}", c, j, now, running=run)


@ref
@pytest.mark.parametrize("lay", gw.NAMED)
def test_preemption_against_the_reference_code(lay):
    from tests.test_ref_pin import both
    c, j, now, run, pre = gw.preempt_case(61, N=12, J=120, P=1, running=40, layout=lay)
    both(f"wide GRES preempt {lay}", c, j, now, running=run, preempt=pre)


@ref
def test_exactly_64_types_against_the_reference_code():
    from tests.test_ref_pin import both
    c, j, now, run = gw.gres_wide_case(80, N=80, J=300, P=2, running=30, layout="uneven", types=64)
    both("64 types", c, j, now, running=run)


# ---------------------------------------------------------------------------------------------------------------------------------
# the calls of tests/test_gpu_gres_wide_calls.py: conditions on the inputs, asserted on the references' answers, so that a case which
# stops reaching its edge fails here and not silently on the device
# ---------------------------------------------------------------------------------------------------------------------------------
WIDE_CALL_LAYOUTS = gw.NAMED + [3, 5]
SUBMIT_LAYOUTS = ["eight_by_8_four_names", "uneven", 3, 5]


@functools.lru_cache(maxsize=None)
def _probe_answers(lay):
    from tests import probe_case as pc
    c, j, p, now, run = gw.probe_case(1, lay)
    return c, j, p, now, run, pc.expected(c, j, p, now, running=run)


@pytest.mark.parametrize("lay", gw.NAMED)
def test_probes_ask_every_kind_of_question(built, lay):
    from tests import probe_case as pc
    c, j, p, now, run, exp = _probe_answers(lay)
    m = pc.outcome_mix(exp, p, now)
    assert p.num_jobs == 32 and m["now"] >= 3 and m["later"] >= 3 and m["resource_no_start"] >= 1 and m["multi_node"] >= 1, m


def test_probes_reach_the_saturated_counts(built):
    """Over the named layouts: a probe is placed on 16 or more slots of one class (64 on one64, 21 on uneven: behind a cycle that filled
    the cluster such a probe starts later, the largest class share of a probe that starts now is 10), a probe's placement holds bit 63,
    and the cycle whose front summaries the probes read started placements of 16 or more slots of one class now (55 on one64, 21 on
    uneven): the 4-bit class counts of the summaries and dips saturate."""
    placed, bit63, cycle_now = {}, False, {}
    for lay in gw.NAMED:
        c, j, p, now, run, exp = _probe_answers(lay)
        cm = gw.class_masks(c.gres)
        placed[lay] = 0
        for i in range(p.num_jobs):
            if exp.start_sec[i] == 0:
                continue
            for x in range(int(exp.place_offsets[i]), int(exp.place_offsets[i + 1])):
                g = int(exp.gres[x])
                bit63 |= bool(g >> 63)
                placed[lay] = max([placed[lay]] + [bin(g & m).count("1") for m in cm])
        cycle_now[lay] = gw.coverage(c, j, pyoracle.select(c, j, now, running=run).placements)["max_class_now"]
    assert max(placed.values()) >= 16 and placed["one64"] >= 16 and placed["uneven"] >= 16, placed
    assert bit63
    assert cycle_now["one64"] >= 16 and cycle_now["uneven"] >= 16, cycle_now


@pytest.mark.parametrize("kind", gw.DIP_KATS)
def test_probe_dip_scenario_is_decided_by_a_saturated_dip(built, kind):
    """gw.probe_dip_kat by hand and on the oracle: the first two probes start now on the node whose time map holds, inside their window,
    an entry with fewer free slots than the front and more than the 15 a nibble can say, and they ask for more than 15."""
    from tests import probe_case as pc
    c, j, rv, p, now, free, want = gw.probe_dip_kat(kind)
    tl = pyoracle.select(c, j, now, reservations=rv).timeline(0)
    got_free = [(int(t), bin(int(g)).count("1")) for t, g in zip(tl["t"], tl["gres"])]
    assert got_free[:len(free)] == free and free[1] == (now + 600, 24)
    exp = pc.expected(c, j, p, now, reservations=rv)
    got = [(int(exp.start_sec[i]), int(exp.node_idx[int(exp.place_offsets[i])])) for i in range(3)]
    assert got == want and list(exp.reason[:3]) == [abi.REASON_NONE] * 3
    need = [max(int(p.gres_spec[i, 0]), int(p.gres_total[i, 0])) for i in range(3)]
    assert 15 < need[0] <= 24 and 15 < need[1] <= 24 < need[2] <= 34 and int(p.time_limit_sec[0]) > 600 >= int(p.time_limit_sec[2])
    assert bin(int(c.gres_slots[1])).count("1") >= need[0], "the other node could take them: a wrong filter changes the answer"


@pytest.mark.parametrize("lay", WIDE_CALL_LAYOUTS)
def test_validity_codes_of_the_wide_queues(lay):
    from tests import valid_pyref
    c, j, now, run = gw.gres_wide_case(1, N=96, J=700, P=2, running=60, layout=lay)
    code, elig = valid_pyref.check(c, j, None)
    n = np.bincount(code, minlength=11)
    assert n[abi.VALID_OK] >= 300 and n[abi.VALID_NOT_ENOUGH_NODES] >= 30, n
    if lay == "one64":                      # 48 nodes of 64 slots cover a request of 255: nothing fails :7283 on its GRES
        assert n[abi.VALID_NO_RESOURCE] == 0
    else:
        assert n[abi.VALID_NO_RESOURCE] >= 5, n


@functools.lru_cache(maxsize=None)
def _submit_answers(lay):
    from tests import submit_pyref as sp
    t, jobs, keys = gw.submit_case(11, lay)
    return t, jobs, keys, sp.run(t, jobs, keys)


@pytest.mark.parametrize("lay", SUBMIT_LAYOUTS)
def test_submit_codes_depend_on_the_walk_order(lay):
    from tests import submit_pyref as sp
    t, jobs, keys, (code, tlo, adm, state) = _submit_answers(lay)
    assert jobs.num_jobs == 600 and 0 < adm < 600
    assert int(jobs.gres_total.max()) <= gw.SUBMIT_COUNT_CAP and int(jobs.gres_spec.max()) <= gw.SUBMIT_COUNT_CAP
    assert t.layout.class_name != sorted(t.layout.class_name), "class-index order and name order must differ on this layout"
    other = sp.run(gw.with_sorted_class_names(t), jobs, keys)[0]
    assert int((other != code).sum()) >= 10, int((other != code).sum())


def test_submit_cases_reach_every_tres_check():
    n = np.zeros(17, np.int64)
    for lay in SUBMIT_LAYOUTS:
        n += np.bincount(_submit_answers(lay)[3][0], minlength=17)
    for c in (abi.SUBMIT_TRES_PER_JOB_BEYOND, abi.SUBMIT_PARTITION_TRES_PER_JOB_BEYOND, abi.SUBMIT_MAX_TRES_PER_USER_BEYOND,
              abi.SUBMIT_MAX_TRES_PER_ACCOUNT_BEYOND):
        assert n[c] >= 3, (abi.SUBMIT_STR[c], n)


@pytest.mark.parametrize("lay", gw.NAMED)
def test_ledger_scenario_carries_wide_masks(built, lay):
    """tests/running_case.scenario over a wide layout: what the four boundaries admit holds masks above bit 31 and bit 63, on rows of
    several nodes; a 32-bit truncation of the gres plane or of a ledger word changes the ledger."""
    from tests import running_case as rc
    cluster, first, cycles = rc.scenario(3, case=gw.wide_case_of(lay))
    assert len(cycles) == 4 and cluster.gres.class_name == gw.make_layout(lay).class_name
    assert sum(c.num_admitted for c in cycles) >= 100 and sum(c.num_retired for c in cycles) >= 20
    assert all(c.num_admitted >= 10 and c.num_retired >= 1 for c in cycles)
    seeded = set(first.ids())
    rows = {r.job_id: r for c in cycles for r in c.after.rows if r.job_id not in seeded}
    assert sum(len(r.allocs) > 1 for r in rows.values()) >= 20
    assert any(a[1]["gres"] >> 32 for r in rows.values() for a in r.allocs)
    assert any(a[1]["gres"] >> 63 for r in rows.values() for a in r.allocs)
