"""The cases of tests/limits_case.py are what tests/test_gpu_limits_seams.py says they are — shown here without a GPU, at the very
sizes the GPU tests use (both read them from cns_limits_shape through limits_case.seam_case):
  * the C++ oracle and the independent restatement tests/limits_pyref.py agree on every reason and on the admitted count;
  * the candidates hold exactly the number of items the seam asks for (5 + 2 level per candidate), and the seam is where it should be;
  * caps bind in the middle (0 < admitted < candidates, three reasons), the expected tail holds, a deep and a shallow account of
    one chain fail at once and the deep one is reported;
  * where a GPU test asserts ordered_fallback == 0, the rounds of the parallel pass — the `bracketing` model of
    tests/test_device_logic_models.py with several records per job, in numpy — decide the case within max_rounds and admit exactly
    the oracle's set: convergence is a condition of the case, not something read off the GPU."""
import functools

import numpy as np
import pytest

from cranesched_amd import limits as lm
from oracle import pyoracle
from tests import limits_case as lc
from tests import limits_pyref
from tests.test_device_logic_models import bracketing, greedy


@functools.lru_cache(maxsize=None)
def _run(key):
    shp = lc.shape()
    kind, args = lc.seam_case(key, shp)
    case = getattr(lc, kind)(*args)
    sel = pyoracle.select(case.cluster, case.jobs, case.now)
    reason, adm, usage = pyoracle.run_limits(case.lay, case.t, case.lj, sel.placements)
    return shp, case, sel.placements, reason, int(adm), usage


@pytest.mark.parametrize("key", lc.ALL_KEYS)
def test_oracle_equals_the_python_restatement_and_the_item_count_is_exact(built, key):
    shp, case, pl, reason, adm, _ = _run(key)
    r_py, a_py = limits_pyref.run(case.lay, case.t, case.lj, pl)
    bad = np.flatnonzero(reason != r_py)
    assert bad.size == 0, f"job {bad[0]}: C++ {lm.LIMIT_REASON_STR[int(reason[bad[0]])]!r}, python {lm.LIMIT_REASON_STR[int(r_py[bad[0]])]!r}"
    assert adm == a_py == int((reason == 0).sum())
    cand = reason != lm.NOT_CANDIDATE
    items = lc.n_items(case.info["levels"][cand])
    if "items" in case.info:                      # every intended candidate started now: the stream is as long as the seam wants it
        assert items == case.info["items"] and int(cand.sum()) == case.info["candidates"]
    if "mask" in case.info:
        assert np.array_equal(cand, case.info["mask"])
    if key in lc.SCAN_KEYS + lc.SMALL_KEYS + ("all_skipped",):      # non-candidates of both kinds, a real permutation
        sel = case.lj.select_index.astype(np.int64)
        pending = pl.reason[sel] != 0
        assert not (pending & cand).any() and np.array_equal(~cand, pending | (case.lj.skip != 0))
        if case.lj.num_jobs > 200:
            assert not np.array_equal(sel, np.arange(len(sel)))
        if key in lc.SCAN_KEYS:
            assert (case.lj.skip != 0).any() and pending.any() and case.lj.num_jobs > shp[5] and 0 < cand.sum() < case.lj.num_jobs // 50


@pytest.mark.parametrize("key", lc.HOT_KEYS)
def test_hot_caps_bind_in_the_middle(built, key):
    shp, case, _, reason, adm, _ = _run(key)
    M = case.info["candidates"]
    assert 0 < adm < M and len(set(reason.tolist()) - {0}) >= 3
    first_reject = int(np.flatnonzero(reason != 0)[0])
    last_admit = int(np.flatnonzero(reason == 0)[-1])
    assert M // 8 <= first_reject < last_admit and last_admit >= M // 2, "admissions and rejections interleave over the middle of the queue"


def test_hot_sizes_sit_on_the_seams(built):
    shp = lc.shape()
    c, nch, batch, rg, _, _ = shp
    items = {k: lc.seam_case(k, shp)[1][0] for k in lc.HOT_KEYS}
    assert [items[k] for k in ("chunk-1", "chunk", "chunk+1", "2chunk+1")] == [c - 1, c, c + 1, 2 * c + 1]
    assert [items[k] for k in ("row-1", "row", "row+1", "2row+1")] == [rg * c - 1, rg * c, rg * c + 1, 2 * rg * c + 1]
    assert all(lc.chunk_len(items[k], shp) == c for k in lc.HOT_KEYS[:9])              # at the floor: a row group is rg * c items
    # level 0: five records of M items each; a segment longer than two row groups holds at least one row group entirely
    assert items["long_segment"] // 5 > 2 * rg * c
    assert lc.chunk_len(items["batch+1"], shp) == c + 1 and (c + 1) % batch != 0
    assert lc.chunk_len(items["batch-1"], shp) % batch == batch - 1 and lc.chunk_len(items["batch-1"], shp) > c
    assert lc.chunk_len(items["batch+1"] - 15, shp) == c, "batch+1 is the smallest such case"


@pytest.mark.parametrize("key", lc.SEGMENT_KEYS)
def test_segment_starts_on_the_last_item_in_front_of_the_boundary(built, key):
    shp, case, pl, reason, adm, _ = _run(key)
    boundary = lc.seam_case(key, shp)[1][0]
    assert boundary in (shp[0], shp[0] * shp[3])
    assert reason[-3:].tolist() == case.info["tail"] == [0, 0, 3] and adm == case.lj.num_jobs - 1     # 3: QosJobsResourceLimit
    # sorted by usage record the user x qos records come first (they start the record array): user 0's, then user 1's
    assert int((case.lj.user == 0).sum()) == boundary - 1 and case.lj.user[-3:].tolist() == [1, 1, 1]
    assert lc.chunk_len(case.info["items"], shp) == shp[0]


@pytest.mark.parametrize("key", lc.HOT_KEYS + lc.SEGMENT_KEYS)
def test_rounds_converge_where_the_gpu_test_asserts_no_fallback(built, key):
    shp, case, pl, reason, adm, _ = _run(key)
    cand = reason != lm.NOT_CANDIDATE
    items = lc.scalar_items(case, pl, cand)
    admitted, rounds = lc.bracket_rounds(items, max_rounds=shp[4])
    assert rounds is not None and rounds <= shp[4] // 4, f"{rounds} rounds: too close to max_rounds = {shp[4]}"
    assert np.array_equal(admitted, reason[cand] == 0), "the model of the rounds admits another set than the oracle"
    print(f"{key}: {int(cand.sum())} candidates, {len(items['job'])} checks, {rounds} rounds")


@pytest.mark.parametrize("seed", range(4))
def test_numpy_rounds_equal_the_scalar_model(seed):
    """bracket_rounds is tests/test_device_logic_models.py::bracketing: same decisions, same number of rounds; several records per
    job, each with its own increment and limit."""
    rng = np.random.default_rng(900 + seed)
    for _ in range(150):
        n, nk = int(rng.integers(1, 60)), int(rng.integers(1, 6))
        keys = [tuple({int(rng.integers(0, nk)), nk + int(rng.integers(0, 2)), 2 * nk + 7}) for _ in range(n)]
        add = rng.integers(1, 9, n).tolist()
        lim = {k: int(rng.integers(4, 60)) for k in range(3 * nk + 10)}
        want, rounds = bracketing(keys, add, lim)
        assert want == greedy(keys, add, lim)
        job = np.array([j for j in range(n) for _ in keys[j]], np.int64)
        key = np.array([k for j in range(n) for k in keys[j]], np.int64)
        items = dict(n=n, job=job, key=key, add=np.asarray(add, np.int64)[job], lim=np.array([lim[k] for k in key], np.int64),
                     use0=np.zeros(len(key), np.int64))
        got, r = lc.bracket_rounds(items)
        assert got.tolist() == want and r == rounds
    # per-record increments: a job that adds 3 to one record and 1 to another
    items = dict(n=3, job=np.array([0, 0, 1, 1, 2, 2]), key=np.array([0, 1, 0, 1, 0, 1]), add=np.array([3, 1, 3, 1, 1, 1]),
                 lim=np.array([4, 2, 4, 2, 4, 2]), use0=np.zeros(6, np.int64))
    got, _ = lc.bracket_rounds(items)
    assert got.tolist() == [True, False, True]


@pytest.mark.parametrize("key", lc.DEEP_KEYS)
def test_deep_tree_reaches_every_level_and_the_deeper_account_wins(built, key):
    shp, case, pl, reason, adm, usage = _run(key)
    t, lj = case.t, case.lj
    cand = reason != lm.NOT_CANDIDATE
    lv = case.info["levels"]
    assert sorted(set(lv[cand].tolist())) == list(range(lm.MAX_CHAIN)), "candidates on accounts of every level"
    assert sorted(set(lv[reason == 0].tolist())) == list(range(lm.MAX_CHAIN)), "admitted jobs on accounts of every level"
    assert 0 < adm < cand.sum() and len(set(reason.tolist()) - {0, 255}) >= 6
    # chains of every length; limits on the two deepest levels
    depth = lambda a: 1 + (depth(int(t.acct_parent[a])) if t.acct_parent[a] != lc.NONE else 0)
    assert sorted({depth(a) for a in range(t.num_accounts)}) == [1, 2, 3, 4, 5, 6]
    assert (t.acct_part_limit.reshape(-1, t.num_partitions)[4:6] != lc.NONE).all()
    assert not t.acct_qos_exists.all() and not t.acct_part_exists.all()
    # usage entries of deep accounts were created by admissions
    assert (usage.acct_part_exists > t.acct_part_exists).any()
    trace = []
    limits_pyref.run(case.lay, t, lj, pl, trace=trace)
    level = lc.DEEP_LEVEL
    both = [(i, r, fails) for i, r, ru, fails in trace
            if ru == 0 and len(fails) >= 2 and level[fails[0][0]] >= 3 and any(level[a] <= 1 and c != fails[0][1] for a, c in fails[1:])]
    assert len(both) >= 20, "jobs in which a deep and a shallow account of the chain fail at once, with different reasons"
    assert all(reason[i] == r == fails[0][1] for i, r, fails in both), "the walk goes from the job's account upward: the deeper account is reported"
    assert any(level[fails[0][0]] >= 4 for _, _, fails in both)


def test_the_oracle_walks_a_chain_of_seven():
    """an engine limit (CNS_LIM_MAX_CHAIN), not parity: the reference's chain is a vector of any length"""
    t = lc.chain_of_seven()
    case = lc.sparse_candidates(1, "stride_lastblock")
    sel = pyoracle.select(case.cluster, case.jobs, case.now)
    z = np.zeros(1, np.uint32)
    lj = lm.LimitJobs(user=z, user_acct=[lm.MAX_CHAIN], account=[lm.MAX_CHAIN], qos=z, partition=z, time_limit_sec=[lc.JOB_L])
    reason, adm, usage = pyoracle.run_limits(case.lay, t, lj, sel.placements)
    assert reason.tolist() == [0] and adm == 1 and usage.acct_qos["jobs_count"].tolist() == [1] * (lm.MAX_CHAIN + 1)


@pytest.mark.parametrize("key", lc.RECORD_KEYS)
def test_many_records_need_a_third_radix_digit(built, key):
    shp, case, pl, reason, adm, usage = _run(key)
    cand = reason != lm.NOT_CANDIDATE
    assert case.info["records"] >= 1 << 16 and case.t.num_users * case.t.num_qos >= 1 << 16
    rec = case.lj.user[cand].astype(np.int64) * case.t.num_qos + case.lj.qos[cand]
    assert rec.min() < 256 and rec.max() >= 1 << 16 and ((rec >= 256) & (rec < 1 << 16)).any()
    assert 1000 < cand.sum() and 0 < adm < cand.sum()
    hi = case.lj.user >= (1 << 16) // case.t.num_qos
    for part in (hi, ~hi):     # per-user caps bind on records below and above the third digit
        assert (reason[part & cand] == 0).any() and np.isin(reason[part & cand], (2, 3)).any()


@pytest.mark.parametrize("key", lc.SCAN_KEYS + lc.SMALL_KEYS)
def test_sparse_queues_admit_and_reject(built, key):
    shp, case, _, reason, adm, _ = _run(key)
    M = case.info["candidates"]
    assert int((reason != lm.NOT_CANDIDATE).sum()) == M
    if M >= 12:
        assert 0 < adm < M
    if key in lc.SCAN_KEYS:
        assert {2, 3} <= set(reason.tolist())


@pytest.mark.parametrize("key", lc.EMPTY_KEYS)
def test_no_candidate_leaves_the_tables_alone(built, key):
    shp, case, _, reason, adm, usage = _run(key)
    assert (reason == lm.NOT_CANDIDATE).all() and adm == 0 and len(reason) == case.lj.num_jobs
    assert usage.same_as(lc.input_usage(case.t))
