"""include/crane_gpu_gate/pending_gate.h: plain C (compiles as C and as C++), the library exports what the header declares, the binding
names the same calls, codes, flags and struct fields, cns_gate_shape returns the constants, the calls fail with a status (never crash)
without a device handle, and the pinned ABI 4 directory is as it was."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "crane_gpu_gate", "pending_gate.h")


def _source():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


@pytest.mark.parametrize("compiler,lang,std", [("gcc", "c", "-std=c99"), ("g++", "c++", "-std=c++17")])
def test_header_compiles_as_c_and_cpp(tmp_path, compiler, lang, std):
    src = tmp_path / ("t.c" if lang == "c" else "t.cpp")
    src.write_text('#include "crane_gpu_gate/pending_gate.h"\n'
                   'int use(cns_handle* h, const cns_gate_jobs* j, const cns_gate_events* e, const cns_gate_out* o) { double ms; uint32_t a, b, c; '
                   'int64_t t = CNS_GATE_TIME_INFINITE_PAST, u = CNS_GATE_TIME_INFINITE_FUTURE; '
                   'return cns_gate_pending(h, 0, j, e, o, &ms) + cns_gate_shape(&a, &b, &c) + (int)CNS_GATE_ARRAY_TASK_LIMIT + (int)CNS_GATE_AP_ALL + (t < u); }\n')
    r = subprocess.run([compiler, "-x", lang, std, "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                        "-o", str(tmp_path / "t.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_header_symbols_exported(built):
    from cranesched_amd import engine
    names = sorted(set(re.findall(r"\b(cns_[a-z_0-9]+)\s*\(", _source())))
    assert names == sorted(engine.GATE_ABI_SYMBOLS) == ["cns_gate_pending", "cns_gate_shape"]
    for n in names:
        assert hasattr(engine.lib(), n), f"{n} declared in pending_gate.h but not exported"


def test_codes_flags_and_structs_follow_the_header():
    from cranesched_amd import abi
    src = _source()
    codes = re.findall(r"\b(CNS_GATE_[A-Z_]+) = (\d+)", src)
    assert len(codes) == 12 and sorted(int(v) for _, v in codes) == list(range(12))
    for name, val in codes:
        assert getattr(abi, name[4:]) == int(val), name
        assert abi.GATE_STR[int(val)] == name[len("CNS_GATE_"):]
    flags = re.findall(r"#define (CNS_GATE_AP_[A-Z_]+) (\d+)u", src)
    assert [n for n, _ in flags] == ["CNS_GATE_AP_HAS_META", "CNS_GATE_AP_HAS_PARENT", "CNS_GATE_AP_COMPLETE", "CNS_GATE_AP_CANCEL", "CNS_GATE_AP_HAS_NEXT",
                                     "CNS_GATE_AP_ALL"]
    for name, val in flags:
        assert getattr(abi, name[4:]) == int(val), name
    assert abi.GATE_AP_ALL == sum(int(v) for n, v in flags if n != "CNS_GATE_AP_ALL")
    assert "#define CNS_GATE_TIME_INFINITE_PAST INT64_MIN" in src and "#define CNS_GATE_TIME_INFINITE_FUTURE INT64_MAX" in src
    for struct, cls, size in (("cns_gate_jobs", abi.CnsGateJobs, 112), ("cns_gate_events", abi.CnsGateEvents, 32), ("cns_gate_out", abi.CnsGateOut, 56)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), src, flags=re.S).group(1)
        fields = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                fields += [f.strip().lstrip("*").strip() for f in re.sub(r"^(const\s+)?\w+\s*\*?", "", decl, count=1).split(",")]
        assert fields == [f[0] for f in cls._fields_], struct
        assert C.sizeof(cls) == size, struct
    assert [f for f, _ in abi.GateJobs._DTYPES] == [f[0] for f in abi.CnsGateJobs._fields_[1:]]
    # the strings the reference writes at JobScheduler.cpp:1381-1392 and Array.cpp:238-256
    assert [abi.GATE_REASON[c] for c in range(2, 12)] == ["Held", "BeginTime", "Dependency", "DependencyNeverSatisfied", "", "ArrayMaterializationComplete",
                                                          "Cancelled", "Deadline", "", "ArrayTaskLimit"]


def test_the_header_carries_the_reference_lines():
    """Every rule of the header's comment names where the reference says so."""
    text = open(HEADER).read()
    for ref_line in (":1353-1372", ":1374-1413", ":1380", ":1384", ":1388", "CtldPublicDefs.cpp:145-160", "CtldPublicDefs.cpp:153", "CtldPublicDefs.cpp:159",
                     "CtldPublicDefs.h:460-462", "CtldPublicDefs.h:464-466", "Array.cpp:683-699", "Array.cpp:236-259", "Array.cpp:240", "Array.cpp:243",
                     "Array.cpp:246", "Array.cpp:249", "Array.cpp:253-256", "SURVEY.md 8(c)"):
        assert ref_line in text, ref_line


def test_shape_and_calls_without_a_handle(built):
    from cranesched_amd import engine
    L = engine.lib()
    a, b, c = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    assert L.cns_gate_shape(C.byref(a), C.byref(b), C.byref(c)) == 0
    assert (a.value, b.value, c.value) == (256, 8, 256)
    a2, b2, c2 = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    assert L.cns_gate_shape(C.byref(a2), C.byref(b2), C.byref(c2)) == 0 and (a2.value, b2.value, c2.value) == (a.value, b.value, c.value)
    assert L.cns_gate_shape(None, None, None) == 0
    assert a.value % 64 == 0 and 2 <= b.value < 64 and c.value >= 64
    assert L.cns_gate_pending(None, C.c_int64(0), None, None, None, None) == -1   # CNS_ERR_INVALID_ARG


def test_the_pinned_directory_is_unchanged():
    assert sorted(os.listdir(os.path.join(ROOT, "include", "crane_gpu"))) == ["node_select.h", "preempt.h", "priority.h", "run_limits.h", "steps.h"]
    src = open(os.path.join(ROOT, "include", "crane_gpu", "node_select.h")).read()
    assert "#define CNS_ABI_VERSION 4u" in src and "pending_gate" not in src
