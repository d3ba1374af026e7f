"""include/crane_gpu_running/running_attrs.h: plain C (compiles as C and as C++), the library exports what the header declares beside
everything it exported before, the binding names the same calls and struct fields with the header's sizes and offsets, the calls fail
with a status (never crash) without a device handle, and the pinned ABI 4 directory and version are as they were."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "crane_gpu_running", "running_attrs.h")
NEW = ["cns_priority_order_resident", "cns_running_advance_attrs", "cns_running_get_attrs", "cns_running_seed_attrs", "cns_running_select_preempt_attrs"]


def _source():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


@pytest.mark.parametrize("compiler,lang,std", [("gcc", "c", "-std=c99"), ("g++", "c++", "-std=c++17")])
def test_header_compiles_as_c_and_cpp(tmp_path, compiler, lang, std):
    src = tmp_path / ("t.c" if lang == "c" else "t.cpp")
    src.write_text('#include "crane_gpu_running/running_attrs.h"\n'
                   'int use(cns_handle* h, const cns_running_soa* rn, const uint32_t* ids, const cns_running_attrs* a, const cns_running_step* s, '
                   'const cns_running_step_out* o, const cns_running_attrs_out* g, const cns_priority_config* c, const cns_prio_pending_soa* pd, uint32_t* ord, '
                   'double* pr, uint64_t* n, const cns_job_soa* j, const cns_preempt_soa* p, cns_placement_soa* pl, cns_preempt_out* po) { '
                   'return cns_running_seed_attrs(h, rn, ids, a) + cns_running_advance_attrs(h, s, a, o) + cns_running_get_attrs(h, g) + '
                   'cns_priority_order_resident(h, 5, c, 3, pd, 9, ord, pr, n) + cns_running_select_preempt_attrs(h, 5, j, p, pl, po); }\n')
    r = subprocess.run([compiler, "-x", lang, std, "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                        "-o", str(tmp_path / "t.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_header_symbols_exported(built):
    from cranesched_amd import engine
    names = sorted(set(re.findall(r"\b(cns_[a-z_0-9]+)\s*\(", _source())))
    assert names == sorted(engine.RUNNING_ATTRS_ABI_SYMBOLS) == NEW
    for n in names:
        assert hasattr(engine.lib(), n), f"{n} declared in running_attrs.h but not exported"
    for m in ("seed_running", "advance_running", "running_attrs", "priority_order_resident", "node_select_preempt_resident"):
        assert callable(getattr(engine.GpuNodeSelector, m))


def test_the_existing_exports_are_a_subset_of_the_new_ones(built):
    """Every symbol of every other header's list is still there; what the library exports with the cns_ prefix is those and the five."""
    from cranesched_amd import engine
    before = set()
    for name in dir(engine):
        if name.endswith("ABI_SYMBOLS") and name != "RUNNING_ATTRS_ABI_SYMBOLS":
            before |= set(getattr(engine, name))
    assert len(before) > 80 and not before & set(NEW)
    for n in before:
        assert hasattr(engine.lib(), n), n
    if shutil.which("nm") is None:
        pytest.skip("no nm")
    out = subprocess.run(["nm", "-D", "--defined-only", engine.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split() and line.split()[-1].startswith("cns_") and " T " in line}
    assert before <= exported and exported - before == set(NEW)


def test_structs_follow_the_header():
    from cranesched_amd import abi
    src = _source()
    for struct, cls, size in (("cns_running_attrs", abi.CnsRunningAttrs, 40), ("cns_running_attrs_out", abi.CnsRunningAttrsOut, 80)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), src, flags=re.S).group(1)
        fields = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                fields += [f.strip().lstrip("*").strip() for f in re.sub(r"^(const\s+)?\w+\s*\*?", "", decl, count=1).split(",")]
        assert fields == [f[0] for f in cls._fields_], struct
        assert C.sizeof(cls) == size, struct
        assert [getattr(cls, f).offset for f, _ in cls._fields_] == [8 * i for i in range(len(cls._fields_))], struct


def test_struct_offsets_as_the_c_compiler_lays_them_out(tmp_path):
    from cranesched_amd import abi
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    lines = []
    for struct, cls in (("cns_running_attrs", abi.CnsRunningAttrs), ("cns_running_attrs_out", abi.CnsRunningAttrsOut)):
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (struct, struct))
        lines += ['printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (struct, f, struct, f) for f, _ in cls._fields_]
    src = tmp_path / "o.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "crane_gpu_running/running_attrs.h"\nint main(void) { %s return 0; }\n' % " ".join(lines))
    exe = tmp_path / "o"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    for struct, cls in (("cns_running_attrs", abi.CnsRunningAttrs), ("cns_running_attrs_out", abi.CnsRunningAttrsOut)):
        assert int(got[struct]) == C.sizeof(cls)
        for f, _ in cls._fields_:
            assert int(got[f"{struct}.{f}"]) == getattr(cls, f).offset, f"{struct}.{f}"


def test_calls_without_a_handle(built):
    from cranesched_amd import engine
    L = engine.lib()
    assert L.cns_running_seed_attrs(None, None, None, None) == -1   # CNS_ERR_INVALID_ARG
    assert L.cns_running_advance_attrs(None, None, None, None) == -1
    assert L.cns_running_get_attrs(None, None) == -1
    assert L.cns_priority_order_resident(None, C.c_int64(0), None, C.c_uint32(0), None, C.c_uint64(0), None, None, None) == -1
    assert L.cns_running_select_preempt_attrs(None, C.c_int64(0), None, None, None, None) == -1


def test_the_header_carries_the_contract_and_the_pinned_surface_is_unchanged():
    text = open(HEADER).read()
    for words in ("LEDGER ORDER", "PLAIN CALLS DROP THE COLUMNS", "CtldPublicDefs.cpp:1901-1902", "JobScheduler.h:74,89", "start_sec = in->now_sec", "must be NULL",
                  "Never a device fault", "Single device only", "CNS_ABI_VERSION stays 4"):
        assert words in text, words
    assert sorted(os.listdir(os.path.join(ROOT, "include", "crane_gpu"))) == ["node_select.h", "preempt.h", "priority.h", "run_limits.h", "steps.h"]
    assert "#define CNS_ABI_VERSION 4u" in open(os.path.join(ROOT, "include", "crane_gpu", "node_select.h")).read()
    assert sorted(os.listdir(os.path.join(ROOT, "include", "crane_gpu_running"))) == ["running.h", "running_attrs.h", "running_preempt.h"]
