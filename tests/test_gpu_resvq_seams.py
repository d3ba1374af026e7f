"""Reservation what-ifs on the GPU at the seams of their device code (tests/resvq_seams.py, built from cns_resvq_shape): times over the
whole signed 64-bit range, chains of 40 reservations per node, empty lists and jobs without an allocation, two | three | four radix
passes over the segment numbers, a sort wider than one step of its scan, and one handle across sizes — every output array for
equality with tests/resvq_pyref.py.  tests/test_resvq_seams.py asserts without a GPU that each scenario is where it claims to be.

The expected answers are computed once per scenario and shared; every call runs twice and both runs must give the same arrays."""
import time

import pytest

from tests import resvq_case as rc
from tests import resvq_seams as rs

pytestmark = pytest.mark.gpu


def _engine(engine_default, seam):
    eng = engine_default(device=0)
    eng.set_nodes(seam.cluster)
    eng.set_resv_query_state(seam.running, seam.resv)
    return eng


def _twice(eng, name):
    seam = rs.case(name)
    got = eng.query_reservations(seam.now, seam.queries)
    rc.same(name, got, rs.expected_of(name))
    again = eng.query_reservations(seam.now, seam.queries)
    rc.same(name + " (again)", again, got)
    return got


@pytest.mark.parametrize("name", ["wide_times", "dense_nodes", "empties", "empties_all_past", "two_passes", "three_passes", "many_tiles", "many_tiles_more",
                                  "three_passes_most", "four_passes"])
def test_seam(engine_default, name):
    t0 = time.perf_counter()
    eng = _engine(engine_default, rs.case(name))
    try:
        rs.expected_of(name)
        t1 = time.perf_counter()
        _twice(eng, name)
        print(f"{name}: {rs.case(name).queries.num_queries} queries, inputs and reference {t1 - t0:.2f} s, two calls and their checks {time.perf_counter() - t1:.2f} s, "
              f"kernels of one call {eng.resv_query_timing()['kernel_ms']:.2f} ms")
    finally:
        eng.close()


def test_one_handle_across_sizes(engine_default):
    """Large -> small -> other tables -> large on ONE handle: the device buffers keep the size of the largest call, and a tail of the
    sorted times, of the histogram or of the chosen slots that a smaller call left behind must never be read."""
    big, small, wide = rs.case("many_tiles"), rs.case("empties"), rs.case("wide_times")
    eng = _engine(engine_default, big)
    try:
        first = _twice(eng, "many_tiles")
        eng.set_nodes(small.cluster)
        eng.set_resv_query_state(small.running, small.resv)
        _twice(eng, "empties")
        past = rs.case("empties_all_past")                       # the same tables: nothing sorted behind a call that sorted a million times
        rc.same("empties_all_past", eng.query_reservations(past.now, past.queries), rs.expected_of("empties_all_past"))
        eng.set_nodes(wide.cluster)
        eng.set_resv_query_state(wide.running, wide.resv)
        _twice(eng, "wide_times")
        eng.set_nodes(big.cluster)
        eng.set_resv_query_state(big.running, big.resv)
        rc.same("many_tiles at the end", _twice(eng, "many_tiles"), first)
    finally:
        eng.close()
