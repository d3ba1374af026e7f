"""include/crane_gpu_running/running.h: plain C (compiles as C and as C++), the library exports what the header declares, the binding
names the same calls and struct fields, cns_running_shape returns the constants, the calls fail with a status (never crash) without a
device handle, and the pinned ABI 4 directory is as it was."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "crane_gpu_running", "running.h")


def _source():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


@pytest.mark.parametrize("compiler,lang,std", [("gcc", "c", "-std=c99"), ("g++", "c++", "-std=c++17")])
def test_header_compiles_as_c_and_cpp(tmp_path, compiler, lang, std):
    src = tmp_path / ("t.c" if lang == "c" else "t.cpp")
    src.write_text('#include "crane_gpu_running/running.h"\n'
                   'int use(cns_handle* h, const cns_running_soa* rn, const uint32_t* ids, const cns_running_step* s, const cns_running_step_out* o, '
                   'const cns_running_ledger* l, cns_running_timing* t) { uint32_t a, b, c, d; '
                   'return cns_running_seed(h, rn, ids) + cns_running_advance(h, s, o) + cns_running_get(h, l) + cns_running_get_timing(h, t) + '
                   'cns_running_shape(&a, &b, &c, &d); }\n')
    r = subprocess.run([compiler, "-x", lang, std, "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                        "-o", str(tmp_path / "t.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_header_symbols_exported(built):
    from cranesched_amd import engine
    names = sorted(set(re.findall(r"\b(cns_running_[a-z_0-9]+)\s*\(", _source())))
    assert names == sorted(engine.RUNNING_ABI_SYMBOLS) == ["cns_running_advance", "cns_running_get", "cns_running_get_timing", "cns_running_seed", "cns_running_shape"]
    for n in names:
        assert hasattr(engine.lib(), n), f"{n} declared in running.h but not exported"
    for m in ("seed_running", "advance_running", "running_ledger", "running_timing", "running_shape"):
        assert callable(getattr(engine.GpuNodeSelector, m))


def test_structs_follow_the_header():
    from cranesched_amd import abi
    src = _source()
    for struct, cls, size in (("cns_running_step", abi.CnsRunningStep, 56), ("cns_running_step_out", abi.CnsRunningStepOut, 24),
                              ("cns_running_ledger", abi.CnsRunningLedger, 128), ("cns_running_timing", abi.CnsRunningTiming, 48)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), src, flags=re.S).group(1)
        fields = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                fields += [f.strip().lstrip("*").strip() for f in re.sub(r"^(const\s+)?\w+\s*\*?", "", decl, count=1).split(",")]
        assert fields == [f[0] for f in cls._fields_], struct
        assert C.sizeof(cls) == size, struct


def test_the_header_carries_the_reference_lines_and_the_canonical_order():
    text = open(HEADER).read()
    for ref_line in ("CranedMetaContainer.cpp:226-277", ":248-253", "JobScheduler.cpp:5318-5425", "CranedMetaContainer.cpp:178-224",
                     "JobScheduler.cpp:1575-1628", "JobScheduler.cpp:6681-6709", ":6685-6686", ":6693-6700", "JobScheduler.h:508-510"):
        assert ref_line in text, ref_line
    assert "Canonicalisation" in text and "LEDGER ORDER" in text and "STABLE" in text and "NOT checked" in text


def test_shape_and_calls_without_a_handle(built):
    from cranesched_amd import engine
    L = engine.lib()
    v = [C.c_uint32(0) for _ in range(4)]
    assert L.cns_running_shape(*[C.byref(x) for x in v]) == 0
    assert [x.value for x in v] == [256, 8, 4096, 256]
    assert L.cns_running_shape(None, None, None, None) == 0
    a, b = C.c_uint32(0), C.c_uint32(0)
    assert L.cns_commit_shape(C.byref(a), C.byref(b)) == 0 and b.value == v[1].value, "the hand-off to the wave at k_cc_check's width"
    assert L.cns_running_seed(None, None, None) == -1        # CNS_ERR_INVALID_ARG
    assert L.cns_running_advance(None, None, None) == -1
    assert L.cns_running_get(None, None) == -1
    assert L.cns_running_get_timing(None, None) == -1


@pytest.mark.gpu
def test_calls_in_the_wrong_order(gpu):
    """CNS_ERR_STATE: a seed before cns_set_nodes, an advance or a get before a seed, an advance after cns_set_running dropped the
    ledger or after num_nodes changed, an admit step without a cycle, cns_select_preempt on tables built on the device."""
    from cranesched_amd import abi
    from cranesched_amd.engine import EngineError, GpuNodeSelector
    from tests import helpers
    cluster, jobs, now, run = helpers.random_case(3, N=24, J=40, P=2, running=6)
    ids = 100 + np.arange(len(run.end_sec), dtype=np.uint32)
    eng = GpuNodeSelector(device=0)

    def state(fn, *a, **kw):
        with pytest.raises(EngineError) as e:
            fn(*a, **kw)
        assert e.value.status == -5, str(e.value)
        return str(e.value)

    assert "before cns_set_nodes" in state(eng.seed_running, run, ids)
    eng.set_nodes(cluster)
    assert "before cns_running_seed" in state(eng.advance_running, [])
    assert "before cns_running_seed" in state(eng.running_ledger)
    eng.seed_running(run, ids)
    assert "needs the results of a successful cycle" in state(eng.advance_running, [], now=now, job_ids=np.arange(jobs.num_jobs, dtype=np.uint32))
    pre = abi.Preempt(qos_preempt=[[]], pd_job_id=np.arange(jobs.num_jobs, dtype=np.uint32), pd_qos=np.zeros(jobs.num_jobs, np.uint32), pd_qos_priority=np.zeros(jobs.num_jobs, np.uint32),
                      pd_priority=np.zeros(jobs.num_jobs),
                      rn_job_id=ids, rn_qos=np.zeros(len(ids), np.uint32), rn_qos_priority=np.zeros(len(ids), np.uint32), rn_start_sec=np.zeros(len(ids), np.int64))
    assert "cns_set_running" in state(eng.node_select_preempt, now, jobs, pre)
    eng.set_running(run)
    assert "before cns_running_seed" in state(eng.advance_running, [])
    eng.seed_running(run, ids)
    eng.advance_running([])
    c2, _, _, _ = helpers.random_case(3, N=25, J=40, P=2, running=0)
    eng.set_nodes(c2)
    assert "before cns_running_seed" in state(eng.advance_running, [])
    assert "before cns_running_seed" in state(eng.running_ledger)
    eng.close()


def test_the_pinned_directory_is_unchanged():
    assert sorted(os.listdir(os.path.join(ROOT, "include", "crane_gpu"))) == ["node_select.h", "preempt.h", "priority.h", "run_limits.h", "steps.h"]
    src = open(os.path.join(ROOT, "include", "crane_gpu", "node_select.h")).read()
    assert "#define CNS_ABI_VERSION 4u" in src and "crane_gpu_running" not in src
