"""include/crane_gpu_usage/usage.h: plain C (compiles as C and as C++), the library exports what the header declares, the binding names the
same calls, constants and struct fields and its struct sizes are the C compiler's sizeof, the calls fail with a status (never crash)
without a device handle, and the pinned ABI 4 directory is as it was."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "crane_gpu_usage", "usage.h")
STRUCTS = ("cns_usage_tables", "cns_usage_jobs", "cns_usage_out", "cns_usage_tables_out", "cns_usage_timing")


def _source():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


@pytest.mark.parametrize("compiler,lang,std", [("gcc", "c", "-std=c99"), ("g++", "c++", "-std=c++17")])
def test_header_compiles_as_c_and_cpp(tmp_path, compiler, lang, std):
    src = tmp_path / ("t.c" if lang == "c" else "t.cpp")
    src.write_text('#include "crane_gpu_usage/usage.h"\n'
                   'int use(cns_handle* h, const cns_usage_tables* t, const cns_usage_jobs* j, const cns_usage_out* o, const cns_usage_tables_out* g) { '
                   'uint32_t a, b, c; cns_usage_timing tm; '
                   'return cns_usage_set_tables(h, t) + cns_usage_apply(h, CNS_USAGE_RELEASE, j, CNS_USAGE_CARRY, o) + cns_usage_apply(h, CNS_USAGE_CHARGE, j, 0, o) + '
                   'cns_usage_get_tables(h, g) + cns_usage_get_timing(h, &tm) + cns_usage_shape(&a, &b, &c) + CNS_USAGE_BIT_ACCT_PART(5) + CNS_USAGE_BIT_QOS + '
                   '(int)(CNS_USAGE_MAX_JOBS > 0); }\n')
    r = subprocess.run([compiler, "-x", lang, std, "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                        "-o", str(tmp_path / "t.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_header_symbols_exported(built):
    from cranesched_amd import engine
    names = sorted(set(re.findall(r"\b(cns_[a-z_0-9]+)\s*\(", _source())))
    assert names == sorted(engine.USAGE_ABI_SYMBOLS) == ["cns_usage_apply", "cns_usage_get_tables", "cns_usage_get_timing", "cns_usage_set_tables",
                                                         "cns_usage_shape"]
    for n in names:
        assert hasattr(engine.lib(), n), f"{n} declared in usage.h but not exported"


def _fields(src, struct):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), src, flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            fields += [re.sub(r"\[.*\]", "", f).strip().lstrip("*").strip() for f in re.sub(r"^(const\s+)?\w+\s*\*?", "", decl, count=1).split(",")]
    return fields


def test_constants_and_structs_follow_the_header(tmp_path):
    from cranesched_amd import abi
    src = _source()
    for name, val in (("RELEASE", 0), ("CHARGE", 1), ("CARRY", 1), ("MAX_JOBS", 16777216), ("BIT_USER_QOS", 0), ("BIT_USER_PART", 1), ("BIT_QOS", 14)):
        assert re.search(r"#define CNS_USAGE_%s %du?\s" % (name, val), src), name
        assert getattr(abi, "USAGE_" + name) == val
    assert "#define CNS_USAGE_BIT_ACCT_QOS(i) (2 + 2 * (i))" in src and "#define CNS_USAGE_BIT_ACCT_PART(i) (3 + 2 * (i))" in src
    assert [abi.usage_bit_acct_qos(i) for i in range(6)] == [2, 4, 6, 8, 10, 12] and [abi.usage_bit_acct_part(i) for i in range(6)] == [3, 5, 7, 9, 11, 13]
    classes = (abi.CnsUsageTables, abi.CnsUsageJobs, abi.CnsUsageOut, abi.CnsUsageTablesOut, abi.CnsUsageTiming)
    for struct, cls in zip(STRUCTS, classes):
        assert _fields(src, struct) == [f[0] for f in cls._fields_], struct
    # sizeof, from the C compiler
    prog = tmp_path / "s.c"
    prog.write_text('#include <stdio.h>\n#include "crane_gpu_usage/usage.h"\nint main(void) { printf("' + " ".join(["%zu"] * len(STRUCTS)) + '\\n", ' +
                    ", ".join(f"sizeof({s})" for s in STRUCTS) + "); return 0; }\n")
    exe = tmp_path / "s"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    sizes = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert sizes == [C.sizeof(c) for c in classes] == [200, 112, 24, 136, 40]   # 6 x 4 + 28 (gres) + 4 (padding) + 18 pointers


def test_calls_without_a_handle_fail_with_a_status(built):
    from cranesched_amd import engine
    L = engine.lib()
    assert L.cns_usage_set_tables(None, None) == -1   # CNS_ERR_INVALID_ARG
    assert L.cns_usage_apply(None, 0, None, 0, None) == -1
    assert L.cns_usage_get_tables(None, None) == -1
    assert L.cns_usage_get_timing(None, None) == -1
    a, b, c = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    assert L.cns_usage_shape(C.byref(a), C.byref(b), C.byref(c)) == 0 and a.value >= 64 and b.value >= a.value and c.value >= 64
    assert L.cns_usage_shape(None, None, None) == 0


def test_the_pinned_directory_is_unchanged():
    assert sorted(os.listdir(os.path.join(ROOT, "include", "crane_gpu"))) == ["node_select.h", "preempt.h", "priority.h", "run_limits.h", "steps.h"]
    src = open(os.path.join(ROOT, "include", "crane_gpu", "node_select.h")).read()
    assert "#define CNS_ABI_VERSION 4u" in src and "crane_gpu_usage" not in src and "cns_usage_" not in src
    assert "crane_gpu_usage" not in open(os.path.join(ROOT, "include", "crane_gpu", "run_limits.h")).read()
