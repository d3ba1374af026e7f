"""include/crane_gpu_probe/probe.h: plain C, compiles as C and as C++, every declared call is exported by the built library and listed
in engine.PROBE_ABI_SYMBOLS, and the calls fail with a status (never crash) without a GPU."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "crane_gpu_probe", "probe.h")


def _declared():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(cns_probe[a-z_0-9]*)\s*\(", src)))


@pytest.mark.parametrize("compiler,lang,std", [("gcc", "c", "-std=c99"), ("g++", "c++", "-std=c++17")])
def test_probe_header_compiles_as_c_and_cpp(tmp_path, compiler, lang, std):
    src = tmp_path / ("t.c" if lang == "c" else "t.cpp")
    src.write_text('#include "crane_gpu_probe/probe.h"\n'
                   'int use(cns_handle* h, const cns_job_soa* p, cns_placement_soa* o) { double ms; return cns_probe(h, p, o, &ms) + '
                   'cns_probe_upload(h, p) + cns_probe_run_resident(h, &ms) + cns_probe_download(h, o); }\n')
    r = subprocess.run([compiler, "-x", lang, std, "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                        "-o", str(tmp_path / "t.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_probe_symbols_exported_and_listed(built):
    from cranesched_amd import abi, engine
    names = _declared()
    assert names == sorted(engine.PROBE_ABI_SYMBOLS) and "cns_probe" in names
    lib = engine.lib()
    for n in names:
        assert hasattr(lib, n), f"{n} declared in probe.h but not exported"
    assert lib.cns_abi_version() == abi.CNS_ABI_VERSION == 4, "the probe calls change no existing struct: the ABI version stays"
    import __graft_entry__ as g
    assert HEADER in g.ENGINE_SRCS and any(s.endswith("probe_kernel.inc") for s in g.ENGINE_SRCS) and any(s.endswith("probe_host.inc") for s in g.ENGINE_SRCS)


def test_probe_calls_reject_null_arguments_without_a_gpu(built):
    from cranesched_amd import abi, engine
    lib = engine.lib()
    jobs = abi.Jobs(partition=[0], time_limit_sec=[60], node_mem=[0], task_cpu_raw=[256], task_mem=[1], node_num=[1], ntasks=[1],
                    ntasks_per_node_min=[1], ntasks_per_node_max=[1])
    out = abi.Placements(1, 1)
    cj, co = jobs.to_c(), out.to_c()
    ms = C.c_double(7.0)
    assert lib.cns_probe(None, C.byref(cj), C.byref(co), C.byref(ms)) == -1       # CNS_ERR_INVALID_ARG
    assert lib.cns_probe(None, None, None, None) == -1
    assert lib.cns_probe_upload(None, C.byref(cj)) == -1
    assert lib.cns_probe_run_resident(None, C.byref(ms)) == -1
    assert lib.cns_probe_download(None, C.byref(co)) == -1
    assert b"cns_probe" in engine.lib().cns_last_error(None)
    assert out.start_sec[0] == 0 and out.node_idx[0] == abi.NODE_NONE, "a refused call writes nothing"


def test_probe_shape_needs_no_handle_and_refuses_a_null_record(built):
    from cranesched_amd import abi, engine
    L = engine.lib()
    assert "cns_probe_shape" in engine.PROBE_ABI_SYMBOLS
    assert L.cns_probe_shape(None) == -1   # CNS_ERR_INVALID_ARG
    rec = abi.CnsProbeShapeInfo()
    C.memset(C.byref(rec), 0xEE, C.sizeof(rec))
    assert L.cns_probe_shape(C.byref(rec)) == 0
    assert rec.pad == 0 and C.sizeof(rec) == 10 * 4 + 8
    s = engine.probe_shape()
    assert s == engine.probe_shape() and isinstance(s, abi.ProbeShape)
    for n in engine.PROBE_DEBUG_ABI_SYMBOLS:
        assert hasattr(L, n), n
    assert L.cns_debug_get_probe_plan(None, None, None) == -1 and L.cns_debug_get_dips(None, None, None, None) == -1


def test_probe_shape_record_mirrors_the_header():
    """abi.CnsProbeShapeInfo field for field against the struct in the header."""
    from cranesched_amd import abi
    src = open(HEADER).read()
    body = re.search(r"typedef struct cns_probe_shape_info \{(.*?)\} cns_probe_shape_info;", src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decls = re.findall(r"(uint32_t|uint64_t)\s+([a-z_0-9]+);", body)
    want = [(f, {C.c_uint32: "uint32_t", C.c_uint64: "uint64_t"}[t]) for f, t in abi.CnsProbeShapeInfo._fields_]
    assert [(n, t) for t, n in decls] == want, decls
    assert abi.ProbeShape._fields == tuple(f for f, _ in want if f != "pad")


def test_the_shipped_probe_figures(built):
    """The constants of the shipped build (csrc/probe_kernel.inc, select_kernels.hip, probe_plan_host.inc, node_select.h), and that the
    record is filled from them: the source names each constant where the record takes it."""
    from cranesched_amd import abi, engine
    from tests import probe_seams as ps
    s = engine.probe_shape()
    assert s == (64, 0xFFFF, 0xFFFF, 15, abi.MAX_GRES_CLASSES, abi.MAX_GRES_NAMES, 64, s.heap_ent_bytes, 0xFFFFFFFF, 1 << 30)
    assert s.heap_ent_bytes % 8 == 0 and 48 <= s.heap_ent_bytes <= 128, "node, slot, ntasks, the cost and one Res"
    assert s == ps.SHIPPED
    csrc = os.path.join(ROOT, "cranesched_amd", "csrc")
    host = open(os.path.join(csrc, "probe_host.inc")).read()
    for line in ("s.block = (u32)kProbeBlock;", "s.dip_cpu_sat = kDipCpuSat; s.dip_mem_sat = kDipMemSat; s.dip_gres_sat = kDipGresSat;",
                 "s.gres_classes = (u32)kMaxClasses; s.gres_names = (u32)kMaxNames;", "s.max_types = CNS_MAX_NODE_TYPES;", "s.loff_clamp = kProbeLoffClamp;"):
        assert line in host, line
    kern = open(os.path.join(csrc, "probe_kernel.inc")).read()
    fits = kern[kern.index("bool probe_fits_dip("):kern.index("void probe_next(")]
    assert "dc != kDipCpuSat" in fits and "dm != kDipMemSat" in fits and fits.count("have != kDipGresSat") == 1 and fits.count("h == kDipGresSat") == 1
    assert "J.L >= (i64)kProbeLoffClamp ? kProbeLoffClamp : (u32)J.L" in kern and "o += (u32)kProbeBlock" in kern and kern.count("i += (u32)kProbeBlock") == 3


def test_python_surface(built):
    from cranesched_amd.engine import GpuNodeSelector
    for m in ("probe", "probe_upload", "probe_run_resident", "probe_download", "probe_timing", "probe_plan", "dips"):
        assert callable(getattr(GpuNodeSelector, m))


def test_nothing_of_the_probe_path_uses_the_oracle():
    """Same rule as tests/test_abi.py: oracle/ is test infrastructure; nothing under cranesched_amd/ or include/ may reference it."""
    for top in ("cranesched_amd", "include"):
        for d, _, files in os.walk(os.path.join(ROOT, top)):
            for f in files:
                if f.endswith((".py", ".hip", ".h", ".inc", ".cpp", ".hpp", "Makefile")):
                    txt = open(os.path.join(d, f), errors="ignore").read()
                    assert not re.search(r"^\s*(from|import)\s+oracle", txt, flags=re.M), f"{f} imports the oracle"
                    assert "liboracle" not in txt and "pyoracle" not in txt and "oracle/" not in txt, f"{f} uses the oracle"
