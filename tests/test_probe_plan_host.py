"""The launch plan of k_probe (cranesched_amd/csrc/probe_plan_host.inc: resident workgroups, heap stride, grid, scratch bytes under the
cap) compiled with g++ and held to its definition (tests/cpp/probe_plan_test.cpp): plain, and once under AddressSanitizer +
UndefinedBehaviorSanitizer as an executable of its own.  And the plan's one home: probe_host.inc launches what the routine says and
has no arithmetic of its own.  No GPU involved."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cranesched_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "probe_plan_test.cpp")


def _read(name):
    return open(os.path.join(CSRC, name)).read()


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def plan_exe(tmp_path_factory, request):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("probe_plan_" + request.param) / "probe_plan_test")
    extra = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "sanitized" else []
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", *extra, "-o", exe, SRC], check=True)
    return exe


def test_grid_stride_and_bytes_hold_their_definition(plan_exe):
    r = subprocess.run([plan_exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_the_plan_file_has_no_hip():
    text = _read("probe_plan_host.inc")
    assert "hip" not in re.sub(r"//[^\n]*", "", text).lower()
    assert '#include "probe_plan_host.inc"' in _read("engine.hip")


def test_probe_host_keeps_no_arithmetic_of_its_own():
    """cns_probe_run_resident takes grid, stride and bytes from cns_probe_plan::plan, with the cap of scratch_cap(); nothing of what the
    routine computes is written out beside it."""
    host = re.sub(r"//[^\n]*", "", _read("probe_host.inc"))
    run = host[host.index("int cns_probe_run_resident("):host.index("int cns_probe_download(")]
    assert run.count("cns_probe_plan::plan(") == 1 and "cns_probe_plan::resident(per_cu, h->num_cus)" in run and "cns_probe_plan::scratch_cap()" in run
    assert "(uint32_t)sizeof(HeapEnt)" in run and "h->rlay.max_np, h->pkmax" in run
    assert "ensure((size_t)L.bytes)" in run and "grid = L.grid; stride = L.stride;" in run
    assert "Q.heap_stride = stride" in run and "dim3((unsigned)grid), dim3(kProbeBlock)" in run
    assert "std::min" not in run and "std::max" not in run and "1ull << 30" not in host and "+ 1u" not in run and "scratch_cap /" not in run
    assert "getenv" not in host, "the environment variable is read in probe_plan_host.inc"
    # the shape names the routine's cap and the entry size it is handed, not copies
    assert "s.scratch_cap = cns_probe_plan::kScratchCap;" in host and "s.heap_ent_bytes = (u32)sizeof(HeapEnt);" in host
