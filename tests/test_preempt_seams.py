"""The seam cases of TryPreempt_'s device form (tests/preempt_seams.py) on the CPU: for every case the oracle equals the independent
Python restatement (and the reference's own code where it is built), and the CONDITION that makes the case a test of its seam holds —
asserted from the restatement's recorder (candidates, applied, chosen, the order) and from the DEVICE's tree source compiled for the host
and fed the recorded operations (tests/host_seg/seg_host.cpp --replay: records and pool nodes the call takes, which form runs out).
tests/test_gpu_preempt_seams.py then holds the engine to the oracle on the same cases."""
import os
import shutil
import subprocess

import pytest

from tests import preempt_seams as ps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEG_FLAGS = ["-O1", "-std=c++17", "-fno-strict-aliasing", "-Wno-unused-function"]


@pytest.fixture(scope="module")
def shape(built):
    from cranesched_amd import engine
    return engine.preempt_shape()


def build_seg_host(tmp, extra=()):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp / "seg_host")
    subprocess.run(["g++", *SEG_FLAGS, *extra, "-o", exe, "seg_host.cpp"], cwd=os.path.join(ROOT, "tests", "host_seg"), check=True)
    return exe


@pytest.fixture(scope="module")
def seg_host(tmp_path_factory):
    return build_seg_host(tmp_path_factory.mktemp("seg_replay"))


def write_call(path, call):
    """One recorded TryPreempt_ call in the format of seg_host --replay.  The cases use cpu, memory and core ids only."""
    def res(r):
        assert not any(r.gres.values())
        w = [sum(1 << (c - 64 * k) for c in r.cores if 64 * k <= c < 64 * k + 64) for k in range(4)]
        return f"{r.cpu} {r.mem} {w[0]} {w[1]} 0 {w[2]} {w[3]}"
    with open(path, "w") as f:
        f.write(f"call {len(call['targets'])} {call['seg_end']}\n")
        for t in call["targets"]:
            f.write(f"target {res(t)}\n")
        for ti, _, st, ed, r, plus in call["ops"]:
            f.write(f"op {ti} {st} {ed} {1 if plus else 0} {res(r)}\n")


def replay(exe, tmp, calls):
    """-> per call a dict of the replay's figures."""
    paths = []
    for n, call in enumerate(calls):
        paths.append(str(tmp / f"call{n}.txt"))
        write_call(paths[-1], call)
    r = subprocess.run([exe, "--replay", *paths], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    out = []
    for line in r.stdout.splitlines():
        w = line.split()
        assert w[0::2][:5] == ["C.used", "C.overflow", "T.used", "T.overflow", "R.nodes"] and w[10] == "satisfied", line
        out.append(dict(c_used=int(w[1]), c_over=int(w[3]), t_used=int(w[5]), t_over=int(w[7]), r_nodes=int(w[9]), satisfied=[int(x) for x in w[11:]]))
    assert len(out) == len(calls)
    return out


@pytest.fixture(scope="module")
def recorded(shape):
    """name -> (case, recorded calls, pyref cycle, out, lists): each case runs through the restatement once."""
    memo = {}

    def get(name):
        if name not in memo:
            cs = ps.case(shape, name)
            memo[name] = (cs,) + ps.call_ops(cs.inputs)
        return memo[name]
    return get


def test_the_case_list_follows_the_shape(shape):
    assert tuple(shape) == (64, 256, 251, 512, 65536) and ps.case_names(shape) == ps.CASE_NAMES
    from cranesched_amd import engine
    assert engine.lib().cns_preempt_shape(None, None, None, None, None) == 0 and shape.rank_sort_max % shape.sort_lanes == 0
    other = type(shape)(32, 96, 100, 64, 4096)
    assert {"nc_31", "nc_32", "nc_33", "nc_95", "nc_96", "nc_97", "nc_128", "list_65"} <= set(ps.case_names(other))


@pytest.mark.parametrize("name", ps.CASE_NAMES)
def test_oracle_equals_the_restatement(built, recorded, name):
    from oracle import pyoracle
    from tests.test_preempt import compare_preempt
    cs, calls, cyc, out, lists = recorded(name)
    c, j, now, run, pre = cs.inputs
    ref = pyoracle.select(c, j, now, running=run, preempt=pre)
    compare_preempt(name, c, j, ref, cyc, out, lists)
    if pyoracle.ref_available():   # ... and the reference's own code
        r2 = pyoracle.select(c, j, now, running=run, preempt=pre, backend="ref")
        assert r2.placements.diff(ref.placements) is None and r2.preempt_out.lists() == ref.preempt_out.lists(), name
        assert r2.preempt_out.cancelled_ids() == ref.preempt_out.cancelled_ids()


def key_of(cyc, ref):
    """The comparator's key without the index (tests/select_pyref.py: try_preempt)."""
    kind, x = ref
    if kind == "rn":
        r = cyc.rn[x]
        return (0 if r["id"] in cyc.preempting else 1, 1, r["qprio"], -r["start"])
    d = cyc.pd[x]
    return (1, 0, d["qprio"], d["prio"])


@pytest.mark.parametrize("name", ps.CASE_NAMES)
def test_the_case_meets_its_condition(shape, recorded, seg_host, tmp_path, name):
    """What each builder's docstring states, from the recorder and the replay (never from the engine)."""
    cs, calls, cyc, out, lists = recorded(name)
    assert "CONDITION" in cs.doc
    figures = replay(seg_host, tmp_path, calls)
    c, j, now, run, pre = cs.inputs
    for n, want in cs.want.items():
        if not isinstance(n, int):
            continue
        assert n < len(calls), (name, "calls", len(calls))
        call, fig = calls[n], figures[n]
        chosen = call["chosen"]
        tag = (name, n, call["candidates"], call["applied"], None if chosen is None else len(chosen), fig)
        assert all(fig["satisfied"]) == (chosen is not None), tag
        if "candidates" in want:
            assert call["candidates"] == want["candidates"], tag
        if "applied" in want:
            assert call["applied"] == want["applied"], tag
        if "chosen" in want:
            assert chosen is not None and len(chosen) == want["chosen"], tag
        if want.get("strict"):
            assert chosen is not None and 0 < len(chosen) < call["applied"] < call["candidates"], tag
        if "trees" in want:
            assert len(call["targets"]) == want["trees"], tag
        if "chosen_set" in want:
            assert chosen is not None and sorted(chosen) == sorted(want["chosen_set"]), tag
        for at in want.get("tie_at", []):
            a, b = call["order"][at - 1], call["order"][at]
            assert key_of(cyc, a) == key_of(cyc, b) and a[1] < b[1], (tag, at, a, b)
        if "first_node_over" in want:
            first = call["nodes"][0]
            on_first = [r for r in call["order"] if first in (cyc.rn[r[1]] if r[0] == "rn" else cyc.pd[r[1]])["allocs"]]
            assert len(on_first) > want["first_node_over"] and len(set(call["order"])) == len(call["order"]), tag
            head = [cyc.rn[r[1]]["allocs"] for r in call["order"][:shape.sort_lanes] if r[0] == "rn"]
            inside = set(call["nodes"])
            assert any(len(a) == 2 and set(a) <= inside for a in head), tag
            assert any(len(a) == 2 and len(set(a) & inside) == 1 for a in head), tag
        if want.get("both_kinds"):
            assert chosen is not None and {k for k, _ in chosen} == {"pd", "rn"}, tag
        if "after" in want:
            before = calls[want["after"]]
            gone = {r for r in before["chosen"] if r[0] == "rn" or cyc.pd[r[1]]["start"] == now}
            assert gone and set(call["order"]) == set(before["order"]) - gone and chosen, tag
        if want.get("replay") == "full":
            assert not fig["c_over"] and shape.compact_records * 9 // 10 < fig["c_used"] <= shape.compact_records, tag
        if want.get("replay") == "over":
            assert fig["c_over"] and not fig["t_over"] and shape.cache_nodes < fig["t_used"] < shape.pool_nodes and chosen, tag
        if want.get("replay") == "pool_deep":
            assert fig["c_over"] and not fig["t_over"] and shape.pool_nodes // 2 < fig["t_used"] < shape.pool_nodes and chosen, tag
        if want.get("replay") == "pool_over":
            assert fig["c_over"] and fig["t_over"] and fig["t_used"] == shape.pool_nodes and fig["r_nodes"] > shape.pool_nodes and chosen, tag
        if "replay" not in want:   # the cases about the candidates keep their trees small: both forms hold them
            assert not fig["c_over"] and not fig["t_over"], tag
    if "node_lists" in cs.want:
        node, n_run, n_rec = cs.want["node_lists"]
        first = calls[0]["job"]
        assert sum(1 for a in run.alloc_node if int(a) == node) == n_run
        assert sum(1 for i in range(first) if node in cyc.pd[i]["nodes"]) == n_rec, name
        starts = {cyc.pd[i]["start"] == now for i in range(first) if node in cyc.pd[i]["nodes"]}
        assert starts == {True, False}, "start-now and backfilled records"
    for i, reason in cs.want.get("reasons", {}).items():
        assert out[i][0] == reason and i not in cyc.cancelled, (name, i, out[i])
    if name == "pending_again":
        assert cyc.cancelled == [] and calls[1]["order"] == [("pd", 1)]


def test_the_recorder_is_off_by_default_and_changes_nothing(built, shape):
    from tests.test_preempt import run_pyref_preempt
    c, j, now, run, pre = ps.case(shape, "multi_k3").inputs
    rec = []
    a = run_pyref_preempt(c, j, now, run, pre)
    b = run_pyref_preempt(c, j, now, run, pre, recorder=rec)
    flat = lambda out: [(reason, start, [(n, t, r.key()) for n, t, r in picks]) for reason, start, picks in out]
    assert a[0].recorder is None and flat(a[1]) == flat(b[1]) and a[2] == b[2] and len(rec) == 1
    call = rec[0]
    assert call["job"] == 0 and len(call["order"]) == call["candidates"] and [(k == "pd", x) for k, x in call["chosen"]] == b[2][0]
    assert {op[0] for op in call["ops"]} == {0, 1, 2} and all(op[2] < op[3] for op in call["ops"])


def test_replay_of_the_overflow_paths_under_the_sanitizers(shape, recorded, tmp_path):
    """The device's tree source, built with AddressSanitizer and UBSan as a stand-alone program, on the calls that run the compressed
    form out of records (compact_over) and the pool out of nodes (pool_over): once a form is full nothing more is written."""
    exe = build_seg_host(tmp_path, ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    for name in ("compact_over", "pool_over"):
        calls = recorded(name)[1]
        fig = replay(exe, tmp_path, calls)[0]
        assert fig["c_over"] and bool(fig["t_over"]) == (name == "pool_over"), (name, fig)
