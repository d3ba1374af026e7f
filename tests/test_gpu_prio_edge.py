"""cns_priority_order on an MI355X against the oracle at the edges of tests/prio_edge.py: priorities as uint64 bit patterns,
the order exactly.  The families are shown to reach their edges, and the oracle is pinned on them to the reference's own code,
by tests/test_prio_edge.py (no GPU needed)."""
import ctypes as C

import numpy as np
import pytest

from cranesched_amd import abi
from cranesched_amd.priority import PrioPending, PrioRunning, PriorityConfig, synth_priority_case
from oracle import pyoracle
from tests import prio_edge as pe

pytestmark = pytest.mark.gpu
CASES = pe.named_cases()
U64_MAX = pe.U64_MAX
CNS_ERR_INVALID_ARG = -1        # include/crane_gpu/node_select.h
assert abi.STATUS_STR[CNS_ERR_INVALID_ARG] == "CNS_ERR_INVALID_ARG"


def _bits(p):
    return np.ascontiguousarray(p, np.float64).view(np.uint64)


def _expected_bytes(pd, rn):
    """The byte formula documented in csrc/priority_host.inc (per pending job 48 + 48 + 16 + 4 + 8 x 32, + 8 with cached
    priorities; per running job 36 + 36 + 4 + 16)."""
    J, R = pd.num_jobs, (rn.num_jobs if rn is not None else 0)
    return J * (48 + 48 + 16 + 4 + 8 * 32) + R * (36 + 36 + 4 + 16) + (J * 8 if pd.cached_priority is not None else 0)


def _check(eng, case, limit=None, tag=""):
    """One call on `eng`, everything compared with the oracle.  Returns (order, priority) of the engine."""
    cfg, A, pd, rn, now = case
    order, prio, nord = eng.priority_order(now, cfg, A, pd, rn, limit=limit)
    ro, rp = pyoracle.priority_order(now, cfg, A, pd, rn)
    ne = np.flatnonzero(_bits(prio) != _bits(rp))
    assert len(ne) == 0, f"{tag}: {len(ne)} priorities differ as bit patterns, first at job {ne[0]}: {prio[ne[0]]!r} vs oracle {rp[ne[0]]!r}"
    no = np.flatnonzero(order != ro)
    assert len(no) == 0, f"{tag}: the order differs at {len(no)} places, first at {no[0]}: job {order[no[0]]} vs oracle {ro[no[0]]}"
    assert nord == min(pd.num_jobs, pd.num_jobs if limit is None else limit), f"{tag}: num_ordered {nord}"
    return order, prio


def _limits(J):
    return sorted({0, 1, max(J - 1, 0), J, J + 1, U64_MAX})


# ---------------------------------------------------------------------------------------------------------------------
# the families
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [0, 777])
@pytest.mark.parametrize("J", pe.TILE_SIZES_SMALL)
def test_gpu_tiles_small(engine_default, J, R):
    eng = engine_default(device=0)
    try:
        case = pe.tiles(J, R, seed=1)
        for limit in _limits(J):
            _check(eng, case, limit=limit, tag=f"tiles J={J} R={R} limit={limit}")
    finally:
        eng.close()


@pytest.mark.parametrize("R", [0, 5000])
@pytest.mark.parametrize("J", pe.TILE_SIZES_LARGE)
def test_gpu_tiles_large(engine_default, J, R):
    """More than 256 tiles: k_sort_rowscan walks its row in several chunks and carries the running total between them."""
    eng = engine_default(device=0)
    try:
        order, prio = _check(eng, pe.tiles(J, R, seed=1), limit=J - 1, tag=f"tiles J={J} R={R}")
        assert pe.tie_share(order, prio) >= 0.20
    finally:
        eng.close()


@pytest.mark.parametrize("name", list(CASES))
def test_gpu_family(engine_default, name):
    eng = engine_default(device=0)
    try:
        case = CASES[name]()
        J = case[2].num_jobs
        for limit in _limits(J):
            _check(eng, case, limit=limit, tag=f"{name} limit={limit}")
    finally:
        eng.close()


def test_gpu_keys_over_a_million_cached_jobs(engine_default):
    """The chosen keys through the multi-chunk row scan: all eight passes move data there."""
    eng = engine_default(device=0)
    try:
        _check(eng, pe.keys(1_200_000, seed=21, R=0), tag="keys J=1.2M")
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# one handle, many calls (CraneCtld keeps one sorter for its lifetime; the engine's buffers only grow)
# ---------------------------------------------------------------------------------------------------------------------
def _sequence(engine_default, steps):
    eng = engine_default(device=0)
    try:
        out = []
        for tag, case in steps:
            out.append(_check(eng, case, tag=tag))
            J = case[2].num_jobs
            t = eng.priority_timing()
            if J == 0:
                assert t["kernels_ms"] == 0 and t["algorithmic_bytes"] == 0, tag
        last = steps[-1][1]
        t = eng.priority_timing()
        assert t["kernels_ms"] > 0, t
        assert t["algorithmic_bytes"] == _expected_bytes(last[2], last[3]), t
        return out
    finally:
        eng.close()


def _empty():
    pd = PrioPending([], [], [], [], [], [], [])
    return PriorityConfig(), 3, pd, None, pe.NOW


def test_gpu_one_handle_large_then_small(engine_default):
    _sequence(engine_default, [("large", pe.tiles(300_000, 5000, seed=2)), ("small", pe.tiles(257, 0, seed=3)),
                               ("one job", pe.tiles(1, 0, seed=4)), ("medium", CASES["wide-mix"]())])


def test_gpu_one_handle_cached_then_null(engine_default):
    with_cached = pe.keys(20_000, seed=5, mixed=True)
    cfg, A, pd, rn, now = pe.keys(20_000, seed=5, mixed=True)
    pd.cached_priority = None
    _sequence(engine_default, [("cached", with_cached), ("NULL", (cfg, A, pd, rn, now)), ("cached again", with_cached),
                               ("NULL, shorter", pe.tiles(4097, 777, seed=6))])


def test_gpu_one_handle_running_then_none(engine_default):
    cfg, A, pd, rn, now = pe.service("mixed", seed=4)
    _sequence(engine_default, [("R > 0", (cfg, A, pd, rn, now)), ("rn = None", (cfg, A, pd, None, now)),
                               ("R > 0 again", pe.service("one_above", seed=4)), ("rn = None, other J", pe.tiles(4095, 0, seed=7))])


def test_gpu_one_handle_keys_then_normal(engine_default):
    pd, rn, now = synth_priority_case(30_000, 4000, 40, seed=8)
    _sequence(engine_default, [("keys", pe.keys(50_000, seed=1)), ("normal", (PriorityConfig(), 40, pd, rn, now)),
                               ("keys, shorter", pe.keys(9000, seed=3, R=0)), ("sparse", CASES["sparse-all_positive"]())])


def test_gpu_one_handle_empty_queue_in_between(engine_default):
    a, b = pe.service("all_above", seed=4), CASES["sparse-both_sides"]()
    cfg, A, pd, rn, now = a
    empty_with_running = (cfg, A, _empty()[2], rn, now)
    _sequence(engine_default, [("a", a), ("J = 0", _empty()), ("b", b), ("J = 0, R > 0", empty_with_running), ("a again", a)])


def test_gpu_one_handle_same_case_twice(engine_default):
    for case in (pe.keys(50_000, seed=2, mixed=True), pe.service("all_above", seed=4), pe.tiles(1_300_001, 5000, seed=1)):
        (o1, p1), (o2, p2) = _sequence(engine_default, [("first", case), ("second", case)])
        assert np.array_equal(_bits(p1), _bits(p2)) and np.array_equal(o1, o2)


# ---------------------------------------------------------------------------------------------------------------------
# argument checks of priority_host.inc: CNS_ERR_INVALID_ARG, and the handle serves the next valid call
# ---------------------------------------------------------------------------------------------------------------------
def _bad_cases():
    def base():
        pd, rn, now = synth_priority_case(300, 50, 5, seed=9)
        return PriorityConfig(), 5, pd, rn, now
    out = {}
    c = base(); c[2].account[7] = 5; out["pending account == num_accounts"] = c
    c = base(); c[2].account[299] = pe.U32_MAX; out["pending account 2^32 - 1"] = c
    c = base(); c[3].account[49] = 5; out["running account == num_accounts"] = c
    c = base(); c[2].total_cpu_raw[0] = -1; out["negative total_cpu_raw"] = c
    c = base(); c[2].total_cpu_raw[150] = -(1 << 63); out["total_cpu_raw int64 min"] = c
    c = base(); c[3].alloc_cpu_raw[3] = -256; out["negative alloc_cpu_raw"] = c
    return out


@pytest.mark.parametrize("what", list(_bad_cases()))
def test_gpu_invalid_values_are_refused_and_the_handle_lives_on(engine_default, what):
    from cranesched_amd.engine import EngineError
    eng = engine_default(device=0)
    try:
        good = pe.tiles(4097, 777, seed=1)
        _check(eng, good, tag="before")
        cfg, A, pd, rn, now = _bad_cases()[what]
        with pytest.raises(EngineError) as e:
            eng.priority_order(now, cfg, A, pd, rn)
        assert e.value.status == CNS_ERR_INVALID_ARG, e.value
        _check(eng, good, tag="after the refusal")
        _check(eng, CASES["wide-mix"](), tag="after the refusal, another case")
    finally:
        eng.close()


@pytest.mark.parametrize("field", ["submit_sec", "qos_priority", "partition_priority", "node_num", "total_cpu_raw", "total_mem", "account",
                                   "r:start_sec", "r:qos_priority", "r:partition_priority", "r:node_num", "r:alloc_cpu_raw", "r:alloc_mem",
                                   "r:account", "order_out", "priority_out", "num_ordered", "cfg", "pd"])
def test_gpu_a_missing_array_is_refused_and_the_handle_lives_on(engine_default, field):
    eng = engine_default(device=0)
    try:
        pd, rn, now = synth_priority_case(300, 50, 5, seed=9)
        cfg = PriorityConfig()
        c_cfg, c_pd, c_rn = cfg.to_c(), pd.to_c(), rn.to_c()
        if field.startswith("r:"):
            setattr(c_rn, field[2:], None)
        elif field in c_pd.__class__.__dict__:
            setattr(c_pd, field, None)
        order, prio, nord = np.empty(300, np.uint32), np.empty(300, np.float64), C.c_uint64(77)
        rc = eng._L.cns_priority_order(
            eng._h, C.c_int64(now), None if field == "cfg" else C.byref(c_cfg), C.c_uint32(5), None if field == "pd" else C.byref(c_pd),
            C.byref(c_rn), C.c_uint64(300), None if field == "order_out" else order.ctypes.data_as(C.c_void_p),
            None if field == "priority_out" else prio.ctypes.data_as(C.c_void_p), None if field == "num_ordered" else C.byref(nord))
        assert rc == CNS_ERR_INVALID_ARG, rc
        assert eng._L.cns_last_error(eng._h)
        _check(eng, (cfg, 5, pd, rn, now), tag="after the refusal")
    finally:
        eng.close()
