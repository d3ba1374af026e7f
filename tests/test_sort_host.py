"""The arithmetic of the shared pair sort (cranesched_amd/csrc/sort_host.inc: passes of a key range, tiles, histogram bytes) compiled with
g++ and held to its definitions (tests/cpp/sort_host_test.cpp): plain, and once under AddressSanitizer + UndefinedBehaviorSanitizer as
an executable of its own.  And the sort's one home: every caller goes through the routines of sort_call.inc, none launches the sort's
kernels or counts passes itself.  No GPU involved."""
import glob
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cranesched_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "sort_host_test.cpp")

# caller -> the routine it sorts with, and the pass count it hands over
CALLERS = {
    "priority_host.inc": ("sort_index_pairs(", "J, 8,"),
    "limits_host.inc": ("sort_index_pairs(", "cns_sort::key_passes(h->lim_sp.NR)"),
    "submit_host.inc": ("sort_index_pairs(", "cns_sort::key_passes(NK)"),
    "usage_host.inc": ("sort_index_pairs(", "cns_sort::key_passes(NK)"),
    "running_host.inc": ("sort_pairs(", "cns_sort::key_passes(S)"),
    "resvq_host.inc": ("sort_pairs(", "cns_resvq::seg_passes(Q)"),
}


def _read(name):
    return open(os.path.join(CSRC, name)).read()


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def sort_exe(tmp_path_factory, request):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("sort_host_" + request.param) / "sort_host_test")
    extra = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "sanitized" else []
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", *extra, "-o", exe, SRC], check=True)
    return exe


def test_passes_tiles_and_histogram_hold_their_definitions(sort_exe):
    r = subprocess.run([sort_exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


@pytest.mark.parametrize("name", sorted(CALLERS))
def test_the_caller_uses_the_routines(name):
    """Each of the six host files sorts through the driver, sizes its histogram with hist_bytes and has no pass loop of its own."""
    host = _read(name)
    routine, passes = CALLERS[name]
    assert routine in host and passes in host, name
    assert "cns_sort::hist_bytes(cns_sort::tiles(" in host, name
    assert "++bits" not in host and "rowtot" not in host and "k_sort_" not in host and "k_iota" not in host, name


def test_the_sort_is_launched_from_one_place():
    """Under csrc/ the histogram and the scatter are launched once, the row scan twice (the sort, scan_counts), k_iota once, all in sort_call.inc."""
    count = {k: {} for k in ("k_sort_hist", "k_sort_scatter", "k_sort_rowscan", "k_iota")}
    for path in glob.glob(os.path.join(CSRC, "*")):
        text = open(path).read()
        for k in count:
            n = len(re.findall(r"hipLaunchKernelGGL\(" + k + r"\b", text))
            if n:
                count[k][os.path.basename(path)] = n
    assert count == {"k_sort_hist": {"sort_call.inc": 1}, "k_sort_scatter": {"sort_call.inc": 1}, "k_sort_rowscan": {"sort_call.inc": 2},
                     "k_iota": {"sort_call.inc": 1}}
    engine = _read("engine.hip")
    for inc in ("sort_kernels.inc", "sort_host.inc", "sort_call.inc"):
        assert f'#include "{inc}"' in engine
    assert engine.index('#include "sort_kernels.inc"') < engine.index('#include "priority_kernels.hip"')
    assert "k_sort_" not in _read("priority_kernels.hip")
    assert _read("gate_host.inc").count("scan_counts(") == 1 and _read("running_host.inc").count("scan_counts(") == 5


def test_the_buffer_sets_are_indexed_by_name():
    """No numeric index into d_prio, d_lim, d_limpar or d_step is left (buf_slots.h names the slots); the counts are what they were."""
    for name in ("priority_host.inc", "limits_host.inc", "steps_call.inc"):
        text = _read(name)
        assert not re.search(r"\bp?b\[[0-9]", text) and not re.search(r"d_(prio|lim|limpar|step)\[[0-9]", text), name
    slots = _read("buf_slots.h")
    for prefix, want in (("PR", 27), ("LM", 29), ("LP", 17), ("ST", 13)):
        body = re.search(r"enum \{ (" + prefix + r"_[A-Z0-9]+ = 0,[^}]*" + prefix + r"_COUNT) \};", slots).group(1)
        names = [x.split("=")[0].strip() for x in re.sub(r"//[^\n]*", "", body).split(",")]
        assert names[-1] == prefix + "_COUNT" and len(names) - 1 == want and len(set(names)) == len(names), prefix
