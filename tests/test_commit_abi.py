"""include/crane_gpu_commit/commit_check.h: plain C (compiles as C and as C++), the library exports what the header declares, the binding
names the same calls, codes and struct fields, the calls fail with a status (never crash) without a device handle, and the pinned ABI 4
directory is as it was."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "crane_gpu_commit", "commit_check.h")


def _source():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


@pytest.mark.parametrize("compiler,lang,std", [("gcc", "c", "-std=c99"), ("g++", "c++", "-std=c++17")])
def test_header_compiles_as_c_and_cpp(tmp_path, compiler, lang, std):
    src = tmp_path / ("t.c" if lang == "c" else "t.cpp")
    src.write_text('#include "crane_gpu_commit/commit_check.h"\n'
                   'int use(cns_handle* h, const cns_commit_events* e, const cns_commit_jobs* j, const cns_commit_out* o) { double ms; uint32_t a, b; '
                   'int64_t t = CNS_CC_TIME_INFINITE_PAST; '
                   'return cns_commit_check(h, e, j, o, &ms) + cns_commit_shape(&a, &b) + (int)CNS_COMMIT_WAITING_PREEMPTION + (t < 0); }\n')
    r = subprocess.run([compiler, "-x", lang, std, "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                        "-o", str(tmp_path / "t.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_header_symbols_exported(built):
    from cranesched_amd import engine
    names = sorted(set(re.findall(r"\b(cns_[a-z_0-9]+)\s*\(", _source())))
    assert names == sorted(engine.COMMIT_ABI_SYMBOLS) == ["cns_commit_check", "cns_commit_shape"]
    for n in names:
        assert hasattr(engine.lib(), n), f"{n} declared in commit_check.h but not exported"


def test_codes_and_structs_follow_the_header():
    from cranesched_amd import abi
    src = _source()
    codes = re.findall(r"\b(CNS_COMMIT_[A-Z_]+) = (\d+)", src)
    assert len(codes) == 8 and sorted(int(v) for _, v in codes) == list(range(8))
    for name, val in codes:
        assert getattr(abi, name[4:]) == int(val), name
        assert abi.COMMIT_STR[int(val)] == name[len("CNS_COMMIT_"):]
    assert "#define CNS_CC_TIME_INFINITE_PAST INT64_MIN" in src and abi.CC_TIME_INFINITE_PAST == -(1 << 63)
    for struct, cls, size in (("cns_commit_events", abi.CnsCommitEvents, 72), ("cns_commit_jobs", abi.CnsCommitJobs, 64),
                              ("cns_commit_out", abi.CnsCommitOut, 16)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), src, flags=re.S).group(1)
        fields = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                fields += [f.strip().lstrip("*").strip() for f in re.sub(r"^(const\s+)?\w+\s*\*?", "", decl, count=1).split(",")]
        assert fields == [f[0] for f in cls._fields_], struct
        assert C.sizeof(cls) == size, struct
    # the strings the reference writes at :1518-1552
    assert [abi.COMMIT_REASON[c] for c in range(3, 8)] == ["Resource changed", "Reservation deleted", "Resource", "Reservation changed",
                                                           "Waiting for Preemption"]


def test_calls_without_a_handle_fail_with_a_status(built):
    from cranesched_amd import engine
    L = engine.lib()
    assert L.cns_commit_check(None, None, None, None, None) == -1   # CNS_ERR_INVALID_ARG
    a, b = C.c_uint32(0), C.c_uint32(0)
    assert L.cns_commit_shape(C.byref(a), C.byref(b)) == 0 and a.value >= 64 and 2 <= b.value < 64
    assert L.cns_commit_shape(None, None) == 0


def test_the_pinned_directory_is_unchanged():
    assert sorted(os.listdir(os.path.join(ROOT, "include", "crane_gpu"))) == ["node_select.h", "preempt.h", "priority.h", "run_limits.h", "steps.h"]
    src = open(os.path.join(ROOT, "include", "crane_gpu", "node_select.h")).read()
    assert "#define CNS_ABI_VERSION 4u" in src and "commit_check" not in src
