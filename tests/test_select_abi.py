"""cns_select_shape (include/crane_gpu/node_select.h): the constants at which the selection kernels change path, without a handle and
without a GPU.  The tile figures must be the ones tests/cpp/plan_host_test.cpp pins for the shipped build (the launch plan works on
the same record: the export reads plan_facts(), it keeps no list of its own)."""
import ctypes as C
import os
import re

from tests import select_seams as ss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_call_needs_no_handle_and_refuses_a_null_record(built):
    from cranesched_amd import abi, engine
    L = engine.lib()
    assert "cns_select_shape" in engine.ABI_SYMBOLS and L.cns_abi_version() == abi.CNS_ABI_VERSION == 4
    assert L.cns_select_shape(None) == -1   # CNS_ERR_INVALID_ARG
    rec = abi.CnsSelectShapeInfo()
    C.memset(C.byref(rec), 0xEE, C.sizeof(rec))
    assert L.cns_select_shape(C.byref(rec)) == 0
    for t in (rec.select, rec.pipe, *rec.wide):
        assert 0 < t.num_widths <= abi.SHAPE_MAX_WIDTHS and all(w == 0 for w in t.widths[t.num_widths:]), "unused widths are zero"
    assert C.sizeof(rec) == 12 * 4 + 6 * (2 + abi.SHAPE_MAX_WIDTHS) * 4 + 4 * 4
    s = engine.select_shape()
    assert s == engine.select_shape() and isinstance(s, abi.SelectShape)


def test_the_record_mirrors_the_header():
    """abi.CnsSelectShapeInfo field for field against the struct in the header."""
    from cranesched_amd import abi
    src = open(os.path.join(ROOT, "include", "crane_gpu", "node_select.h")).read()
    body = re.search(r"typedef struct cns_select_shape_info \{(.*?)\} cns_select_shape_info;", src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for decl in re.findall(r"(?:uint32_t|cns_tile_shape)\s+([^;]+);", body) for n in re.findall(r"([a-z_0-9]+)(?:\[\d+\])?\s*(?:,|$)", decl.strip())]
    assert names == [f for f, _ in abi.CnsSelectShapeInfo._fields_], names
    assert int(re.search(r"#define CNS_SHAPE_MAX_WIDTHS (\d+)u", src).group(1)) == abi.SHAPE_MAX_WIDTHS


def test_the_shipped_figures(built):
    from cranesched_amd import engine
    s = engine.select_shape()
    # the kernels' constants of the shipped build (csrc/engine_params.h, select_kernels.hip, pipe_kernel.inc, wide_kernel.inc)
    assert s[:12] == (64, 1008, 8, 8, 32, 33, 256, 32, 64, 8, 32, 19)
    assert s.lds_heap == s.max_upd + 1 and s.multi_k <= s.pipe_max_k and s.wide_window + 8 < 64
    for r in (s.pipe_ring, s.wide_task_ring, s.pipe_xring, s.alloc_cache):
        assert r & (r - 1) == 0, "rings and the cache are indexed with a mask"
    # tests/cpp/plan_host_test.cpp: shipped()
    assert s.select == (448, (1, 3, 10, 19, 28, 37)) and s.pipe == (512, (1, 4, 8, 16))
    assert s.wide == ((64, (4096, (1, 2, 4, 8, 16))), (32, (2048, (1, 2, 4, 8))), (16, (1024, (1, 2, 4, 8))), (8, (512, (1, 2, 4, 8))))
    assert s.sel_dip_max_npl in s.select.widths and s.select.widths[-1] > s.sel_dip_max_npl
    assert s == ss.SHIPPED


def test_the_tile_figures_are_the_ones_plan_host_test_pins():
    """The literals of shipped() in tests/cpp/plan_host_test.cpp, read from its source."""
    src = open(os.path.join(ROOT, "tests", "cpp", "plan_host_test.cpp")).read()
    s = ss.SHIPPED
    ints = lambda text: tuple(int(x) for x in re.findall(r"\d+", text))
    sel = re.search(r"f\.select\.lanes = (\d+);.*?f\.select\.widths = \{([^}]*)\}", src)
    pipe = re.search(r"f\.pipe\.lanes = (\d+);.*?f\.pipe\.widths = \{([^}]*)\}", src)
    assert (int(sel.group(1)), ints(sel.group(2))) == s.select and (int(pipe.group(1)), ints(pipe.group(2))) == s.pipe
    waves = ints(re.search(r"waves\[4\] = \{([^}]*)\}", src).group(1))
    lanes = ints(re.search(r"lanes\[4\] = \{([^}]*)\}", src).group(1))
    common = ints(re.search(r"b\.tiles\.widths = \{([^}]*)\}", src).group(1))
    extra = ints(re.search(r"f\.wide\[0\]\.tiles\.widths\.push_back\((\d+)\)", src).group(1))
    assert tuple((w, (l, common + (extra if i == 0 else ()))) for i, (w, l) in enumerate(zip(waves, lanes))) == s.wide
