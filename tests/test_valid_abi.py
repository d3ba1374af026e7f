"""include/crane_gpu_valid/validity.h: plain C (compiles as C and as C++), the library exports what the header declares, the binding names
the same calls and codes, the calls fail with a status (never crash) without a device handle, and the pinned ABI 4 directory is as it was."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "crane_gpu_valid", "validity.h")


def _source():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


@pytest.mark.parametrize("compiler,lang,std", [("gcc", "c", "-std=c99"), ("g++", "c++", "-std=c++17")])
def test_header_compiles_as_c_and_cpp(tmp_path, compiler, lang, std):
    src = tmp_path / ("t.c" if lang == "c" else "t.cpp")
    src.write_text('#include "crane_gpu_valid/validity.h"\n'
                   'int use(cns_handle* h, const cns_job_soa* j, const cns_validity_out* o) { double ms; uint32_t a, b; '
                   'return cns_validate_jobs(h, j, o, &ms) + cns_validate_shape(&a, &b) + (int)CNS_VALID_NOT_ENOUGH_NODES; }\n')
    r = subprocess.run([compiler, "-x", lang, std, "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                        "-o", str(tmp_path / "t.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_header_symbols_exported(built):
    from cranesched_amd import engine
    names = sorted(set(re.findall(r"\b(cns_[a-z_0-9]+)\s*\(", _source())))
    assert names == sorted(engine.VALID_ABI_SYMBOLS) == ["cns_validate_jobs", "cns_validate_shape"]
    for n in names:
        assert hasattr(engine.lib(), n), f"{n} declared in validity.h but not exported"


def test_codes_and_struct_follow_the_header():
    from cranesched_amd import abi
    src = _source()
    codes = re.findall(r"\b(CNS_VALID_[A-Z_]+) = (\d+)", src)
    assert len(codes) == 11 and sorted(int(v) for _, v in codes) == list(range(11))
    for name, val in codes:
        assert getattr(abi, name[4:]) == int(val), name
        assert abi.VALID_STR[int(val)] == name[len("CNS_VALID_"):]
    body = re.search(r"typedef struct cns_validity_out \{(.*?)\} cns_validity_out;", src, flags=re.S).group(1)
    assert re.findall(r"\*\s*([a-z_]+);", body) == [f[0] for f in abi.CnsValidityOut._fields_]
    assert C.sizeof(abi.CnsValidityOut) == 16


def test_calls_without_a_handle_fail_with_a_status(built):
    from cranesched_amd import engine
    L = engine.lib()
    assert L.cns_validate_jobs(None, None, None, None) == -1   # CNS_ERR_INVALID_ARG
    a, b = C.c_uint32(0), C.c_uint32(0)
    assert L.cns_validate_shape(C.byref(a), C.byref(b)) == 0 and a.value >= 64 and b.value >= 64
    assert L.cns_validate_shape(None, None) == 0


def test_the_pinned_directory_is_unchanged():
    assert sorted(os.listdir(os.path.join(ROOT, "include", "crane_gpu"))) == ["node_select.h", "preempt.h", "priority.h", "run_limits.h", "steps.h"]
    src = open(os.path.join(ROOT, "include", "crane_gpu", "node_select.h")).read()
    assert "#define CNS_ABI_VERSION 4u" in src and "validate" not in src and "validity" not in src
