"""cns_serial_shape (include/crane_gpu/node_select.h): the loop shapes of the serial protocol (k_mem, k_giant), without a handle and
without a GPU.  The figures must be the ones tests/cpp/plan_host_test.cpp pins for the shipped build and the ones the source names."""
import ctypes as C
import os
import re

from tests import serial_seams as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cranesched_amd", "csrc")


def test_the_call_needs_no_handle_and_refuses_a_null_record(built):
    from cranesched_amd import abi, engine
    L = engine.lib()
    assert "cns_serial_shape" in engine.ABI_SYMBOLS
    assert L.cns_serial_shape(None) == -1   # CNS_ERR_INVALID_ARG
    rec = abi.CnsSerialShapeInfo()
    C.memset(C.byref(rec), 0xEE, C.sizeof(rec))
    assert L.cns_serial_shape(C.byref(rec)) == 0
    assert C.sizeof(rec) == 12 * 4
    s = engine.serial_shape()
    assert s == engine.serial_shape() and isinstance(s, abi.SerialShape) and all(0 < v < 0xEEEEEEEE for v in s)


def test_the_record_mirrors_the_header():
    """abi.CnsSerialShapeInfo field for field against the struct in the header."""
    from cranesched_amd import abi
    src = open(os.path.join(ROOT, "include", "crane_gpu", "node_select.h")).read()
    body = re.search(r"typedef struct cns_serial_shape_info \{(.*?)\} cns_serial_shape_info;", src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for decl in re.findall(r"uint32_t\s+([^;]+);", body) for n in re.findall(r"([a-z_0-9]+)\s*(?:,|$)", decl.strip())]
    assert names == [f for f, _ in abi.CnsSerialShapeInfo._fields_] == list(abi.SerialShape._fields), names


def test_the_shipped_figures(built):
    from cranesched_amd import engine
    s = engine.serial_shape()
    assert s == sr.SHIPPED
    assert s.mem_slots == s.scan_lanes * 64 * s.mem_words and s.giant_mem_slots == s.scan_lanes * 64 * s.giant_mem_words
    assert 64 % s.scan_trip_rows == 0, "a trip's rows never straddle a mask word"
    assert s.helpers_max <= 64, "one answer per lane of the home's tester wave"
    sel = engine.select_shape()
    assert s.select_tile_slots == sel.select.lanes * sel.select.widths[-1]


def test_the_figures_are_the_ones_the_sources_name():
    """The constants by name in wide_kernel.inc, plan_host.inc and engine.hip, and shipped() of tests/cpp/plan_host_test.cpp."""
    s = sr.SHIPPED
    wide, plan, eng = (open(os.path.join(CSRC, f)).read() for f in ("wide_kernel.inc", "plan_host.inc", "engine.hip"))
    const = lambda src, name: int(re.search(r"constexpr u32 " + name + r" = (\d+)u?;", src).group(1))
    assert const(wide, "kWMsTrip") == s.scan_trip_rows and const(wide, "kGiantTrip") == s.helper_trip_slots
    assert const(wide, "kWMemWords") == s.mem_words and const(wide, "kWMemWordsGiant") == s.giant_mem_words
    assert const(wide, "kGiantHelpersMax") == s.helpers_max and const(eng, "kGiantHelperBudget") == s.helper_budget
    assert const(plan, "kGiantMinHelpers") == s.helpers_min and "nh >= kGiantMinHelpers" in plan
    assert "r0 += kWMsTrip" in wide and "o += kGiantTrip * stride" in wide
    test = open(os.path.join(ROOT, "tests", "cpp", "plan_host_test.cpp")).read()
    m = re.search(r"f\.mem_slots = (\d+); f\.giant_mem_slots = (\d+); f\.giant_helpers_max = (\d+); f\.giant_helper_budget = (\d+);", test)
    assert tuple(int(x) for x in m.groups()) == (s.mem_slots, s.giant_mem_slots, s.helpers_max, s.helper_budget)
    assert f"kGiantMinHelpers == {s.helpers_min}" in test
