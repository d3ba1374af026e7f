"""The families of tests/prio_edge.py, made trustworthy on the CPU before tests/test_gpu_prio_edge.py hands them to the engine:
every family reaches the edge it is named for (asserted from oracle output), the oracle agrees on it with the reference's own
MultiFactorPriority (oracle/_ref, bit for bit) and, where a plain-Python walk is cheap, with tests/prio_pyref.py."""
import time

import numpy as np
import pytest

from oracle import pyoracle
from tests import prio_edge as pe

needs_ref = pytest.mark.skipif(not pyoracle.ref_available(), reason="oracle/_ref is not built and the reference tree is absent")
CASES = pe.named_cases()


def _bits(p):
    return np.ascontiguousarray(p, np.float64).view(np.uint64)


def _oracle(case, backend="oracle"):
    cfg, A, pd, rn, now = case
    return pyoracle.priority_order(now, cfg, A, pd, rn, backend=backend)


def _same_as_reference(case):
    """Priorities as bit patterns.  The reference's sort is unstable: with ties its order must be a permutation with non-increasing
    priorities (which fixes the multiset of jobs per priority value); without ties it must be the oracle's order exactly."""
    o_a, p_a = _oracle(case)
    o_b, p_b = _oracle(case, backend="ref")
    assert np.array_equal(_bits(p_a), _bits(p_b)), "priorities differ as bit patterns"
    J = len(p_a)
    assert np.array_equal(np.sort(o_b), np.arange(J)), "the reference's order is no permutation"
    s_a, s_b = p_a[o_a.astype(np.int64)], p_b[o_b.astype(np.int64)]
    assert (s_b[:-1] >= s_b[1:]).all(), "the reference's order is not by descending priority"
    assert np.array_equal(_bits(s_a), _bits(s_b)), "the sorted priority sequences differ"   # same multiset per value, same places
    if pe.tie_share(o_a, p_a) == 0.0:
        assert np.array_equal(o_a, o_b), "no ties, yet the order differs"
    else:     # inside one priority value the jobs are the same set
        for lo, hi in _tie_groups(s_a):
            assert np.array_equal(np.sort(o_a[lo:hi]), np.sort(o_b[lo:hi]))


def _tie_groups(sorted_prio):
    cut = np.flatnonzero(sorted_prio[1:] != sorted_prio[:-1]) + 1
    edges = np.concatenate([[0], cut, [len(sorted_prio)]])
    return [(int(a), int(b)) for a, b in zip(edges[:-1], edges[1:]) if b - a > 1]


def _pyref(case):
    from tests.test_priority import _pyref_run
    cfg, A, pd, rn, now = case
    return _pyref_run(now, cfg, pd, rn)


def _same_as_pyref(case):
    o_a, p_a = _oracle(case)
    o_c, p_c = _pyref(case)
    assert np.array_equal(_bits(p_a), _bits(np.array(p_c, np.float64))), "priorities differ as bit patterns"
    assert o_a.tolist() == o_c


# ---------------------------------------------------------------------------------------------------------------------
# tiles
# ---------------------------------------------------------------------------------------------------------------------
def test_tile_sizes_sit_on_the_seams_they_are_named_for():
    assert [pe.ntiles(J) for J in pe.TILE_SIZES_LARGE] == [256, 257, 318, 513]
    assert set(pe.TILE_SIZES_SMALL) == {255, 256, 257, 4095, 4096, 4097}
    assert 256 < pe.ntiles(pe.TILE_SIZES_LARGE[2]) <= 320 and pe.ntiles(pe.TILE_SIZES_LARGE[3]) > 2 * pe.ROWSCAN_CHUNK
    assert pe.TILE_SIZES_LARGE[3] > 2_097_153 + 2000


@pytest.mark.parametrize("R", [0, 777])
@pytest.mark.parametrize("J", pe.TILE_SIZES_SMALL + (40_000,))
def test_tiles_tie_and_agree_with_the_reference_build(J, R):
    case = pe.tiles(J, R, seed=1)
    order, prio = _oracle(case)
    share = pe.tie_share(order, prio)
    print(f"tiles J={J} R={R}: tie share {share:.3f}, {len(np.unique(prio))} distinct priorities")
    assert share >= 0.20
    assert len(np.unique(prio)) >= 6          # ... and still something to sort
    if pyoracle.ref_available():
        _same_as_reference(case)


@pytest.mark.parametrize("J", pe.TILE_SIZES_LARGE)
def test_large_tiles_tie_across_every_seam(J):
    """At full size only the oracle runs (its time is printed: the multi-million-job GPU cases were sized by it)."""
    case = pe.tiles(J, 5000, seed=1)
    t0 = time.perf_counter()
    order, prio = _oracle(case)
    dt = time.perf_counter() - t0
    print(f"tiles J={J}: oracle {dt * 1e3:.0f} ms = {dt * 1e9 / J:.0f} ms per million jobs")
    assert pe.tie_share(order, prio) >= 0.20
    p = prio[order.astype(np.int64)]
    # the attributes are drawn independently per job, so a value that occurs hundreds of times occurs in tiles of every chunk
    assert len(np.unique(prio)) * 100 <= J
    half = J // 2
    assert len(np.intersect1d(prio[:pe.TILE], prio[half:])) >= 6 and len(np.intersect1d(prio[-pe.TILE:], prio[:half])) >= 6
    assert (p[:-1] >= p[1:]).all()


# ---------------------------------------------------------------------------------------------------------------------
# keys
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in CASES if n.startswith("keys")])
def test_keys_cover_every_digit_of_every_byte(name):
    cfg, A, pd, rn, now = CASES[name]()
    order, prio = _oracle((cfg, A, pd, rn, now))
    cached = pd.cached_priority != 0.0
    assert np.array_equal(_bits(prio[cached]), _bits(pd.cached_priority[cached])), "a cached priority was not kept verbatim"
    cov = pe.digit_coverage(prio[cached])
    print(f"{name}: digits per key byte (low to high) {cov}")
    assert min(cov) >= 200
    assert not np.isnan(prio).any()
    v = prio[cached]
    assert (v < 0).any() and np.isposinf(v).any() and np.isneginf(v).any() and (v == pe.DBL_MAX).any() and (v == -pe.DBL_MAX).any()
    assert ((np.abs(v) < np.finfo(np.float64).tiny) & (v > 0)).any() and ((np.abs(v) < np.finfo(np.float64).tiny) & (v < 0)).any()
    if name.endswith("mixed"):
        assert 0.4 < cached.mean() < 0.6 and (prio[~cached] >= 0).all()
    else:
        assert cached.all()
    # runs of equal values over the tile seams of the INPUT, and the order keeps them in input order
    for t in range(1, pe.ntiles(pd.num_jobs)):
        if t * pe.TILE + 300 <= pd.num_jobs and cached[t * pe.TILE - 1] and cached[t * pe.TILE]:
            assert prio[t * pe.TILE - 1] == prio[t * pe.TILE]
    p = prio[order.astype(np.int64)]
    same = p[:-1] == p[1:]
    assert same.sum() > 1000 and (order[:-1][same] < order[1:][same]).all()


@needs_ref
@pytest.mark.parametrize("name", [n for n in CASES if n.startswith("keys")])
def test_keys_agree_with_the_reference_build(name):
    _same_as_reference(pe.small(name))


# ---------------------------------------------------------------------------------------------------------------------
# service
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", pe.SERVICE_REGIMES)
def test_service_regime_holds_and_shows_in_the_priorities(regime):
    """The regime from the per-account sums; sv_min as the priorities show it: with weights (0, 1, 0, 0, 0) a job's priority IS
    1 - (its account's sum - sv_min) / (sv_max - sv_min)."""
    case = pe.service(regime, seed=5, fair_only=True)
    cfg, A, pd, rn, now = case
    acc, sv_min, sv_max = pe.account_values(cfg, pd, rn, now)
    print(f"{regime}: sums {sorted(acc.values())}")
    assert pe.service_regime_of(acc) == regime
    counts = np.bincount(rn.account, minlength=A)
    assert counts.tolist() == pe.service_counts(regime)
    assert max(counts) > 4000 and any(c % 8 for c in counts if c > 1000)
    if regime == "all_above":
        assert sv_min == pe.SV_MIN_START and min(acc.values()) > pe.SV_MIN_START
        assert len(acc) == A - 1            # the last id is on no job
    else:
        assert sv_min == min(acc.values()) == 0.0 and {0, 1, 7, 8, 9, 13} <= set(counts.tolist())
    order, prio = _oracle(case)
    expect = np.array([1.0 - (acc[int(a)] - sv_min) / (sv_max - sv_min) for a in pd.account])
    assert np.array_equal(_bits(prio), _bits(expect)), "the oracle's priorities do not show these sums and this sv_min"
    if regime == "all_above":     # a minimum that started at DBL_MAX would give the lowest account the factor 1.0
        assert prio.max() < 1.0
        lowest = min(acc, key=acc.get)
        assert 0.0 < prio[pd.account == lowest][0] < 1.0


@pytest.mark.parametrize("name", [n for n in CASES if n.startswith("service")])
def test_service_agrees_with_the_python_restatement(name):
    _same_as_pyref(CASES[name]())


@needs_ref
@pytest.mark.parametrize("name", [n for n in CASES if n.startswith("service")])
def test_service_agrees_with_the_reference_build(name):
    _same_as_reference(CASES[name]())


# ---------------------------------------------------------------------------------------------------------------------
# sparse
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", pe.SPARSE_VARIANTS)
def test_sparse_ids_are_sparse_and_one_sided(variant):
    case = pe._with_cfg(pe.sparse(variant, seed=7), pe.PriorityConfig(**pe.FAIR_ONLY))
    cfg, A, pd, rn, now = case
    used = pe.used_ids(pd, rn)
    assert A == 100_000 and len(used) == (50 if variant == "both_sides" else 30)
    assert 0 not in used and A - 1 in used
    run_only, pend_only = np.setdiff1d(rn.account, pd.account), np.setdiff1d(pd.account, rn.account)
    assert len(run_only) == 20 and len(pend_only) == (20 if variant == "both_sides" else 0)
    assert A > 10 * pd.num_jobs
    acc, sv_min, sv_max = pe.account_values(cfg, pd, rn, now)
    assert sorted(acc) == used.tolist()
    order, prio = _oracle(case)
    expect = np.array([1.0 - (acc[int(a)] - sv_min) / (sv_max - sv_min) for a in pd.account])
    assert np.array_equal(_bits(prio), _bits(expect))
    if variant == "all_positive":   # only an absent id's 0.0 could bring sv_min to 0, and then no priority would reach 1.0
        assert sv_min == min(acc.values()) > 0.0
        assert prio.max() < 1.0 or (pd.account[prio == 1.0] == min(acc, key=acc.get)).all()
        assert sv_min < pe.SV_MIN_START
    else:
        assert sv_min == 0.0 and (prio[np.isin(pd.account, pend_only)] == 1.0).all()


@pytest.mark.parametrize("name", [n for n in CASES if n.startswith("sparse")])
def test_sparse_agrees_with_the_python_restatement(name):
    _same_as_pyref(CASES[name]())


@needs_ref
@pytest.mark.parametrize("name", [n for n in CASES if n.startswith("sparse")])
def test_sparse_agrees_with_the_reference_build(name):
    _same_as_reference(CASES[name]())


# ---------------------------------------------------------------------------------------------------------------------
# wide
# ---------------------------------------------------------------------------------------------------------------------
def test_wide_variants_reach_their_domains():
    w = lambda v: pe.wide(v, seed=8)
    cfg, A, pd, rn, now = w("mem53")
    assert (pd.total_mem > 1 << 53).all() and (pd.total_mem.astype(np.float64).astype(np.uint64) != pd.total_mem).any()
    cfg, A, pd, rn, now = w("mem63")
    assert (pd.total_mem >= 1 << 63).sum() > 100 and (rn.alloc_mem >= 1 << 63).sum() > 50 and pd.total_mem.max() == pe.U64_MAX
    cfg, A, pd, rn, now = w("age53")
    assert cfg.max_age_sec == pe.U64_MAX and ((now - pd.submit_sec) > 1 << 53).sum() > 100
    cfg, A, pd, rn, now = w("age63")
    assert cfg.max_age_sec == pe.U64_MAX and (pd.submit_sec > now).sum() > 100     # u64(now - submit) >= 2^63
    cfg, A, pd, rn, now = w("cpu62")
    assert pd.total_cpu_raw.max() == 1 << 62 and pd.total_cpu_raw.min() == 0 and (rn.alloc_cpu_raw > 1 << 61).any()
    for v, f in (("qos32", "qos_priority"), ("part32", "partition_priority"), ("nodes32", "node_num")):
        cfg, A, pd, rn, now = w(v)
        assert getattr(pd, f).max() == pe.U32_MAX and getattr(pd, f).min() == 0 and getattr(rn, f).max() == pe.U32_MAX
    assert [w(v)[0].max_age_sec for v in ("max_age_0", "max_age_1", "max_age_max")] == [0, 1, pe.U64_MAX]
    cfg, A, pd, rn, now = w("future_submit")
    assert (pd.submit_sec > now).sum() > 100 and cfg.max_age_sec < 1 << 32
    cfg, A, pd, rn, now = w("future_start")
    assert (rn.start_sec > now).sum() > 20
    cfg, A, pd, rn, now = w("r50j")
    assert rn.num_jobs == 50 * pd.num_jobs
    assert all(getattr(w("w_zero")[0], f) == 0 and getattr(w("w_max")[0], f) == pe.U32_MAX for f in pe._ALL_WEIGHTS)


def test_all_weights_zero_is_the_identity_order():
    case = pe.wide("w_zero", seed=8)
    order, prio = _oracle(case)
    assert (_bits(prio) == 0).all(), "every priority is +0.0"
    assert np.array_equal(order, np.arange(len(prio)))


def test_wide_edges_show_in_the_priorities():
    """Each edge changes the oracle's answer against the same case without it — a variant that the formula ignored would test nothing."""
    base = pe.wide("max_age_max", seed=8)
    _, p_base = _oracle(base)
    for v in ("mem53", "mem63", "age53", "age63", "cpu62", "qos32", "part32", "nodes32", "max_age_0", "max_age_1", "future_start", "w_max"):
        _, p = _oracle(pe.wide(v, seed=8))
        assert not np.array_equal(_bits(p), _bits(p_base)), v
        assert np.isfinite(p).all() and (p >= 0).all(), v


@pytest.mark.parametrize("name", [n for n in CASES if n.startswith("wide")])
def test_wide_agrees_with_the_python_restatement(name):
    _same_as_pyref(CASES[name]())


@needs_ref
@pytest.mark.parametrize("name", [n for n in CASES if n.startswith("wide")])
def test_wide_agrees_with_the_reference_build(name):
    _same_as_reference(CASES[name]())
