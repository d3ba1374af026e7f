"""The snapshot layout (cranesched_amd/csrc/snapshot_host.inc: the union-find over shared nodes, the refusals group by group, the slot list, the
virtual partitions of the reservations, the node types, the tag ranges, the running allocations grouped by slot — what cns_set_nodes,
cns_set_reservations and cns_set_running derive on the host) compiled with g++ and compared field by field with the walk it replaced, which
tests/cpp/snapshot_host_test.cpp carries.  No GPU involved: the builders are arithmetic on the caller's arrays, and the limits of the build
are parameters that the test reaches with snapshots of a few nodes."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def snapshot_host(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("snapshot_host") / "snapshot_host_test")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "snapshot_host_test.cpp")], check=True)
    return exe


def test_snapshot_layout_is_the_walk_it_replaced(snapshot_host):
    r = subprocess.run([snapshot_host], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
