"""The run-limit admission (cns_apply_run_limits: csrc/limits_kernels.hip, csrc/limits_host.inc) on the seams of its device code,
against the C++ oracle: reasons, admitted count, all five usage tables, the exists arrays, the candidate count and the resident
re-run (tests/test_run_limits.py::_gpu_vs_oracle; integers, no tolerance), in both modes — the bracketing rounds over the sorted
items and CNS_LIMITS_MODE=seq, the ordered single-wave kernel.

Every size comes from cns_limits_shape (tests/limits_case.py::seam_case); what each case is — where its items fall, that caps bind in
its middle, that the rounds converge so that "no ordered fallback" may be asserted — is shown on the CPU in tests/test_limits_case.py.
  1. item chunks: min_item_chunk - 1, + 0, + 1, 2 x + 1 items on ONE engine, up and down again
  2. the carry scan's row groups (carry_row_chunks chunks each): the same around one and two row groups, a record whose segment
     is longer than two row groups, a segment that starts on the last item in front of a chunk / a row group
  3. a chunk length above the floor that is no multiple of `batch`: a masked partial batch in the middle of the stream
  4. the block scan: more than scan_jobs jobs with few candidates in four lane patterns, 1 / 255 / 256 / 257 jobs, no candidate, no job
  5. account chains of every length up to CNS_LIM_MAX_CHAIN (a job record's slots 11 - 14), and one account more: refused
  6. more than 65 536 usage records: a third radix pass over the item keys"""
import functools

import numpy as np
import pytest

from cranesched_amd import abi, limits as lm
from cranesched_amd.engine import EngineError
from oracle import pyoracle
from tests import limits_case as lc
from tests.test_run_limits import _gpu_vs_oracle

pytestmark = pytest.mark.gpu
MODES = ["parallel", "ordered"]
ERR_UNSUPPORTED = -4
assert abi.STATUS_STR[ERR_UNSUPPORTED] == "CNS_ERR_UNSUPPORTED"


def _mode(monkeypatch, mode):
    if mode == "ordered":
        monkeypatch.setenv("CNS_LIMITS_MODE", "seq")
    else:
        monkeypatch.delenv("CNS_LIMITS_MODE", raising=False)


@functools.lru_cache(maxsize=None)
def _case(kind, args):
    """the case and the oracle's answer, computed once and shared by both modes"""
    case = getattr(lc, kind)(*args)
    sel = pyoracle.select(case.cluster, case.jobs, case.now)
    return case, (sel.placements,) + tuple(pyoracle.run_limits(case.lay, case.t, case.lj, sel.placements))


def _check(eng, key, mode, converges=False):
    """one case on the open engine; converges: the CPU suite has shown that the rounds decide it"""
    shp = eng.limits_shape()
    kind, args = lc.seam_case(key, shp)
    case, ref = _case(kind, args)
    fallback = (mode == "ordered") if converges else None
    reason, usage = _gpu_vs_oracle(None, case.cluster, case.jobs, case.now, case.lay, case.t, case.lj, f"{key} {kind}{args} {mode}",
                                   expect_fallback=fallback, eng=eng, ref=ref)
    tm = eng.limit_timing()
    if mode == "ordered" and tm["candidates"]:
        assert tm["ordered_fallback"] == 1 and tm["rounds"] == 0
    if converges and mode == "parallel":
        assert tm["ordered_fallback"] == 0 and 0 < tm["rounds"] <= shp[4]
    print(f"{key} {kind}{args} {mode}: {tm['candidates']} candidates, {tm['admitted']} admitted, rounds {tm['rounds']}, "
          f"ordered_fallback {tm['ordered_fallback']}, prep {tm['prep_ms']:.3f} ms, admit {tm['admit_ms']:.3f} ms")
    return case, ref, reason, usage


def _one(engine_default, monkeypatch, key, mode, converges=False):
    _mode(monkeypatch, mode)
    eng = engine_default(device=0)
    try:
        return _check(eng, key, mode, converges)
    finally:
        eng.close()


def test_shape_is_the_kernels(engine_default):
    eng = engine_default(device=0)
    try:
        shp = eng.limits_shape()
    finally:
        eng.close()
    c, nch, batch, rg, maxr, scan = shp
    assert shp == lc.shape() and c % batch == 0 and nch % rg == 0 and c >= batch > 1 and maxr >= 8 and scan % 256 == 0


# ---- 1. item chunks ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_item_chunk_seams_up_and_down_on_one_engine(engine_default, monkeypatch, mode):
    """a small batch behind a large one must not see the streams, the tails or the item count the large one left"""
    _mode(monkeypatch, mode)
    eng = engine_default(device=0)
    try:
        keys = ["chunk-1", "chunk", "chunk+1", "2chunk+1"]
        for key in keys + keys[::-1]:
            _check(eng, key, mode, converges=True)
    finally:
        eng.close()


# ---- 2. the carry scan's row groups ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("key", ["row-1", "row", "row+1", "2row+1"])
def test_carry_row_group_seams(engine_default, monkeypatch, key, mode):
    _one(engine_default, monkeypatch, key, mode, converges=True)


@pytest.mark.parametrize("mode", MODES)
def test_segment_longer_than_two_row_groups(engine_default, monkeypatch, mode):
    """five records of M items each, M > 2 row groups: at least one row group lies inside a segment and adds through"""
    case, _, _, _ = _one(engine_default, monkeypatch, "long_segment", mode, converges=True)
    c, _, _, rg, _, _ = lc.shape()
    assert case.info["candidates"] > 2 * rg * c and (case.info["levels"] == 0).all()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("key", lc.SEGMENT_KEYS)
def test_segment_that_starts_on_the_last_item_in_front_of_a_boundary(engine_default, monkeypatch, key, mode):
    case, _, reason, _ = _one(engine_default, monkeypatch, key, mode, converges=True)
    assert reason[-3:].tolist() == [0, 0, 3] == case.info["tail"]          # 3: QosJobsResourceLimit


# ---- 3. a chunk length that is no multiple of the batch --------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("key", ["batch+1", "batch-1"])
def test_chunk_length_that_is_no_multiple_of_the_batch(engine_default, monkeypatch, key, mode):
    case, _, _, _ = _one(engine_default, monkeypatch, key, mode, converges=True)
    shp = lc.shape()
    c, nch, batch = shp[:3]
    length = -(-case.info["items"] // nch)
    assert length > c and length % batch != 0
    assert length % batch == (1 if key == "batch+1" else batch - 1)


# ---- 4. the block scan -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("key", lc.SCAN_KEYS)
def test_block_scan_past_one_count_per_thread(engine_default, monkeypatch, key, mode):
    case, _, _, _ = _one(engine_default, monkeypatch, key, mode)
    assert case.lj.num_jobs > lc.shape()[5]


@pytest.mark.parametrize("mode", MODES)
def test_block_scan_small_queues_on_one_engine(engine_default, monkeypatch, mode):
    _mode(monkeypatch, mode)
    eng = engine_default(device=0)
    try:
        for key in lc.SMALL_KEYS:
            _check(eng, key, mode)
    finally:
        eng.close()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("key", lc.EMPTY_KEYS)
def test_no_candidate_and_no_job(engine_default, monkeypatch, key, mode):
    case, _, reason, usage = _one(engine_default, monkeypatch, key, mode)
    assert len(reason) == case.lj.num_jobs and (reason == lm.NOT_CANDIDATE).all()
    assert usage.same_as(lc.input_usage(case.t))


def test_queue_behind_an_empty_one_on_one_engine(engine_default, monkeypatch):
    """no candidate, then candidates, then none again: the counters of the empty run are its own"""
    _mode(monkeypatch, "parallel")
    eng = engine_default(device=0)
    try:
        for key in ("all_skipped", "J=256", "J=0", "chunk+1", "all_skipped"):
            case, _, reason, usage = _check(eng, key, "parallel")
            if key in lc.EMPTY_KEYS:
                tm = eng.limit_timing()
                assert tm["candidates"] == tm["admitted"] == tm["rounds"] == tm["ordered_fallback"] == 0
                assert (reason == lm.NOT_CANDIDATE).all() and usage.same_as(lc.input_usage(case.t))
    finally:
        eng.close()


# ---- 5. depth ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("key", lc.DEEP_KEYS)
def test_deep_tree(engine_default, monkeypatch, key, mode):
    _one(engine_default, monkeypatch, key, mode)


@pytest.mark.parametrize("mode", MODES)
def test_chain_of_seven_is_refused_and_the_engine_goes_on(engine_default, monkeypatch, mode):
    _mode(monkeypatch, mode)
    eng = engine_default(device=0)
    try:
        kind, args = lc.seam_case("deep:1", eng.limits_shape())
        case, _ = _case(kind, args)
        eng.set_nodes(case.cluster)
        with pytest.raises(EngineError) as e:
            eng.set_run_limits(lc.chain_of_seven())
        assert e.value.status == ERR_UNSUPPORTED
        _check(eng, "deep:1", mode)
    finally:
        eng.close()


# ---- 6. record count ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("key", lc.RECORD_KEYS)
def test_more_than_65536_usage_records(engine_default, monkeypatch, key, mode):
    case, _, _, _ = _one(engine_default, monkeypatch, key, mode)
    assert case.info["records"] >= 1 << 16
