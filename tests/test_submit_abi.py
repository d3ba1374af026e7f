"""include/crane_gpu_submit/submit_limits.h: plain C (compiles as C and as C++), the library exports what the header declares, the binding
names the same calls, codes and struct fields, the calls fail with a status (never crash) without a device handle, and the pinned ABI 4
directory is as it was."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "crane_gpu_submit", "submit_limits.h")


def _source():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


@pytest.mark.parametrize("compiler,lang,std", [("gcc", "c", "-std=c99"), ("g++", "c++", "-std=c++17")])
def test_header_compiles_as_c_and_cpp(tmp_path, compiler, lang, std):
    src = tmp_path / ("t.c" if lang == "c" else "t.cpp")
    src.write_text('#include "crane_gpu_submit/submit_limits.h"\n'
                   'int use(cns_handle* h, const cns_submit_tables* t, const cns_job_soa* j, const cns_submit_keys* k, const cns_submit_out* o) { '
                   'uint32_t a, b, c; cns_submit_timing tm; int64_t m = CNS_SUBMIT_JOB_MAX_TIME_LIMIT_SEC; '
                   'return cns_set_submit_limits(h, t) + cns_check_submissions(h, j, k, CNS_SUBMIT_CARRY, o) + cns_get_submit_usage(h, 0, 0, 0, 0, 0, 0, 0, 0) + '
                   'cns_get_submit_timing(h, &tm) + cns_submit_shape(&a, &b, &c) + (int)CNS_SUBMIT_MAX_TRES_PER_ACCOUNT_BEYOND + (m > 0) + '
                   '(int)(CNS_SUBMIT_MAX_JOBS > 0); }\n')
    r = subprocess.run([compiler, "-x", lang, std, "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                        "-o", str(tmp_path / "t.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_header_symbols_exported(built):
    from cranesched_amd import engine
    names = sorted(set(re.findall(r"\b(cns_[a-z_0-9]+)\s*\(", _source())))
    assert names == sorted(engine.SUBMIT_ABI_SYMBOLS) == ["cns_check_submissions", "cns_get_submit_timing", "cns_get_submit_usage",
                                                          "cns_set_submit_limits", "cns_submit_shape"]
    for n in names:
        assert hasattr(engine.lib(), n), f"{n} declared in submit_limits.h but not exported"


def _fields(src, struct):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), src, flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            fields += [re.sub(r"\[.*\]", "", f).strip().lstrip("*").strip() for f in re.sub(r"^(const\s+)?\w+\s*\*?", "", decl, count=1).split(",")]
    return fields


def test_codes_and_structs_follow_the_header():
    from cranesched_amd import abi, submit
    src = _source()
    codes = re.findall(r"\b(CNS_SUBMIT_[A-Z_]+) = (\d+)", src)
    assert len(codes) == 17 and sorted(int(v) for _, v in codes) == list(range(17))     # dense from 0
    for name, val in codes:
        assert getattr(abi, name[4:]) == int(val), name
        assert abi.SUBMIT_STR[int(val)] == name[len("CNS_SUBMIT_"):]
    assert len(abi.SUBMIT_STR) == 17
    assert "#define CNS_SUBMIT_JOB_MAX_TIME_LIMIT_SEC INT64_C(315576000000)" in src and abi.SUBMIT_JOB_MAX_TIME_LIMIT_SEC == 315576000000
    assert "#define CNS_SUBMIT_CARRY 1u" in src and abi.SUBMIT_CARRY == 1
    assert "#define CNS_SUBMIT_MAX_JOBS 16777216u" in src and abi.SUBMIT_MAX_JOBS == 16777216
    for struct, cls, size in (("cns_submit_tables", abi.CnsSubmitTables, 200), ("cns_submit_keys", abi.CnsSubmitKeys, 48),
                              ("cns_submit_out", abi.CnsSubmitOut, 24), ("cns_submit_timing", abi.CnsSubmitTiming, 56)):
        assert _fields(src, struct) == [f[0] for f in cls._fields_], struct
        assert C.sizeof(cls) == size, struct
    for struct, dt, size in (("cns_submit_qos", submit.SUBMIT_QOS_DT, 416), ("cns_submit_part_limit", submit.SUBMIT_PART_LIMIT_DT, 136)):
        assert _fields(src, struct) == list(dt.names), struct
        assert dt.itemsize == size
    # the reference's CraneErrCode names (src/Utilities/PublicHeader/protos/PublicDefs.proto), its spelling of TIMIT included
    assert abi.SUBMIT_ERR_NAME[abi.SUBMIT_TIME_LIMIT_BEYOND] == "ERR_TIME_TIMIT_BEYOND" and abi.SUBMIT_ERR_NAME[abi.SUBMIT_OK] == "SUCCESS"
    assert abi.SUBMIT_ERR_NAME[abi.SUBMIT_PARTITION_MAX_SUBMIT_JOBS_PER_ACCOUNT] == "ERR_PARTITION_MAX_SUBMIT_JOBS_PER_ACCOUNT"


def test_calls_without_a_handle_fail_with_a_status(built):
    from cranesched_amd import engine
    L = engine.lib()
    assert L.cns_set_submit_limits(None, None) == -1   # CNS_ERR_INVALID_ARG
    assert L.cns_check_submissions(None, None, None, 0, None) == -1
    assert L.cns_get_submit_usage(None, None, None, None, None, None, None, None, None) == -1
    assert L.cns_get_submit_timing(None, None) == -1
    a, b, c = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    assert L.cns_submit_shape(C.byref(a), C.byref(b), C.byref(c)) == 0 and a.value >= 64 and b.value >= a.value and 8 <= c.value <= 256
    assert L.cns_submit_shape(None, None, None) == 0


def test_the_pinned_directory_is_unchanged():
    assert sorted(os.listdir(os.path.join(ROOT, "include", "crane_gpu"))) == ["node_select.h", "preempt.h", "priority.h", "run_limits.h", "steps.h"]
    src = open(os.path.join(ROOT, "include", "crane_gpu", "node_select.h")).read()
    assert "#define CNS_ABI_VERSION 4u" in src and "submit_limits" not in src and "cns_submit" not in src
    assert "submit_limits" not in open(os.path.join(ROOT, "include", "crane_gpu", "run_limits.h")).read()
