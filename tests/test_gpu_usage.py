"""Releases and charges on the usage tables (include/crane_gpu_usage/usage.h, csrc/usage_kernels.inc) on the GPU against
tests/usage_pyref.py, the statement-by-statement restatement of DoFreeResource_ / DoMallocResource_ (AccountMetaContainer.cpp:1067-1208):
the five usage tables, their submit counts, the nested exists bytes, the entity bits and both per-job masks for equality (all integers,
no tolerance).  The named cases of tests/usage_case.py at the smallest shapes that can still go wrong, the seams read from
cns_usage_shape, a saturating prefix, charges (creating entities, refused at a 32-bit wrap), CNS_USAGE_CARRY, seeded random sweeps
for both ops, independence of the other calls, and the input rules."""
import numpy as np
import pytest

from cranesched_amd import abi
from cranesched_amd.engine import EngineError
from tests import usage_case as uc
from tests import usage_pyref as up

pytestmark = pytest.mark.gpu


def _run(engine_default, case, what):
    """The calls of a case in sequence on one engine, each against pyref from the state the header says it starts from.
    -> [(not_found, over_free)] of pyref per call (None for a refused one)."""
    t, steps = case
    eng = engine_default(device=0)
    masks = []
    try:
        eng.set_usage_tables(t)
        assert eng.usage_tables().differences(t.state()) == [], f"{what}: the tables as set"
        cur = t.state()
        for i, (op, js, carry) in enumerate(steps):
            src = cur if carry else t.state()
            call = eng.release_usage if op == uc.REL else eng.charge_usage
            try:
                want, wnf, wof = up.apply(t, src, op, js)
            except up.Refused as r:
                with pytest.raises(EngineError) as e:
                    call(js, carry=carry)
                assert e.value.status == r.status, f"{what}, call {i}"
                assert eng.usage_tables().differences(cur) == [], f"{what}, call {i}: a refused call changed the tables"
                masks.append(None)
                continue
            nf, of, clean = call(js, carry=carry)
            bad = np.flatnonzero((nf != wnf) | (of != wof))
            assert len(bad) == 0, (f"{what}, call {i}: {len(bad)} of {js.num_jobs} jobs differ, first job {int(bad[0])}: not_found {int(nf[bad[0]]):#x} want "
                                   f"{int(wnf[bad[0]]):#x}, over_free {int(of[bad[0]]):#x} want {int(wof[bad[0]]):#x}")
            assert clean == int(np.count_nonzero((wnf | wof) == 0)), f"{what}, call {i}: num_clean"
            assert eng.usage_tables().differences(want) == [], f"{what}, call {i}"
            cur = want
            masks.append((wnf, wof))
        return masks, eng.usage_timing()
    finally:
        eng.close()


def test_one_job(engine_default):
    (m,), _ = _run(engine_default, uc.one_job(), "one job")
    assert not m[0].any() and not m[1].any()


def test_exact_fit_erases_and_the_second_job_stays_clean(engine_default):
    case = uc.exact_fit()
    (m,), _ = _run(engine_default, case, "T == val")
    assert not m[0].any() and not m[1].any()
    want, _, _ = up.apply(case[0], case[0].state(), uc.REL, case[1][0][1])
    assert not want.user_qos_exists[0] and not want.acct_part_exists[0] and want.user_qos_exists[1]      # the touched nested records are gone


@pytest.mark.parametrize("component", range(17), ids=uc.COMPONENTS)
def test_one_unit_over_in_one_component(engine_default, component):
    (m,), _ = _run(engine_default, uc.one_over(component), f"T == val + 1 in {uc.COMPONENTS[component]}")
    every = sum(1 << b for b in (0, 1, 2, 3, 14))
    assert m[0].tolist() == [0, 0] and m[1].tolist() == [0, every]


def test_middle_job_trips_and_the_permutation(engine_default):
    a, b = uc.middle_trips((0, 1, 2)), uc.middle_trips((0, 2, 1))
    (ma,), _ = _run(engine_default, a, "middle job trips")
    (mb,), _ = _run(engine_default, b, "the same jobs permuted")
    back = [0, 2, 1]                                               # the permuted call's masks by the first call's job numbers
    assert not (np.array_equal(ma[0], mb[0][back]) and np.array_equal(ma[1], mb[1][back])), "the two orders must give different masks"
    wa, _, _ = up.apply(a[0], a[0].state(), uc.REL, a[1][0][1])
    wb, _, _ = up.apply(b[0], b[0].state(), uc.REL, b[1][0][1])
    assert wa.differences(wb) == []                                # and identical tables (both engine runs were held to these)
    assert ma[1][1] and ma[0][2] and not ma[0][1]                  # over-free in the middle, the keys gone behind it


def test_global_qos_record_over_freed_twice(engine_default):
    (m,), _ = _run(engine_default, uc.qos_over_freed_twice(), "qos over-freed twice")
    assert m[1].tolist() == [0, 1 << 14, 1 << 14, 1 << 14] and not m[0].any()


@pytest.mark.parametrize("name", ["class_the_record_lacks", "absent_user_entity", "user_acct_none", "saturating_prefix", "charge_creates", "charge_wraps"])
def test_named_case(engine_default, name):
    masks, _ = _run(engine_default, getattr(uc, name)(), name)
    if name == "saturating_prefix":
        assert masks[0][1][1] and masks[0][0][2]                   # the second job over-frees although the record holds UINT64_MAX
    if name == "charge_wraps":
        assert [m is None for m in masks] == [False, True, True, False]
    if name == "user_acct_none":
        assert masks[0][0].tolist() == [2, 0]


@pytest.mark.parametrize("length", [1, 6])
def test_chain_lengths(engine_default, length):
    _run(engine_default, uc.chain(length), f"a chain of {length}")


def test_one_record_at_the_item_chunk_seams(engine_default):
    eng = engine_default(device=0)
    try:
        _, item_chunk, _ = eng.usage_shape()
    finally:
        eng.close()
    for J in (item_chunk - 1, item_chunk, item_chunk + 1, 2 * item_chunk + 1):
        for exact in (False, True):
            (m,), tm = _run(engine_default, uc.one_record(J, seed=J, exact=exact), f"one QoS record, {J} jobs, exact={exact}")
            assert tm["items"] == J and tm["records"] == 1
            assert m[1][-1] and not m[1][0]                        # the fold trips inside the segment
        (m,), _ = _run(engine_default, uc.one_nested_record(J, seed=J), f"one nested record, {J} jobs")
        assert m[0][-1] & 1 and not m[0][0] & 1 and not m[1].any()      # erased by an exact fit: the jobs behind find the key gone, nobody over-frees


def test_every_job_on_records_of_its_own(engine_default):
    eng = engine_default(device=0)
    try:
        job_chunk, _, _ = eng.usage_shape()
    finally:
        eng.close()
    J = job_chunk + 1
    _, tm = _run(engine_default, uc.own_records(J), "records of their own")
    assert tm["items"] == 4 * J and tm["records"] == 4 * J


def test_carry_lanes_seam(engine_default):
    """More scan workgroups than the carry kernel has lanes: each lane takes two of them."""
    eng = engine_default(device=0)
    try:
        _, item_chunk, carry_lanes = eng.usage_shape()
    finally:
        eng.close()
    J = (item_chunk * carry_lanes) // 15 + 70
    t, js = uc.deep_contested(J)
    js.user_acct[:] = js.user                                      # 15 items for every job
    js.skip[:] = 0
    (m,), tm = _run(engine_default, (t, [(uc.REL, js, False)]), "carry lanes seam")
    assert tm["items"] > item_chunk * carry_lanes and tm["items"] == 15 * J
    assert m[0].any() and m[1].any() and ((m[0] | m[1]) == 0).any()


def test_carry(engine_default):
    masks, _ = _run(engine_default, uc.carry_sequence(), "release, charge, release; then without the flag")
    assert all(m is not None for m in masks)


@pytest.mark.parametrize("op", [uc.REL, uc.CHG], ids=["release", "charge"])
@pytest.mark.parametrize("seed", [1, 2])
def test_random_sweep(engine_default, op, seed):
    t, js = uc.random_case(seed, 400, op)
    (m,), _ = _run(engine_default, (t, [(op, js, False)]), f"random sweep {seed}")
    if op == uc.REL:
        assert m[0].any() and m[1].any() and ((m[0] | m[1]) == 0).any()


def test_repeated_runs_are_identical(engine_default):
    t, js = uc.random_case(7, 400, uc.REL)
    eng = engine_default(device=0)
    try:
        eng.set_usage_tables(t)
        first = eng.release_usage(js) + (eng.usage_tables(),)
        for _ in range(3):
            nf, of, clean = eng.release_usage(js)
            assert np.array_equal(nf, first[0]) and np.array_equal(of, first[1]) and clean == first[2] and eng.usage_tables().same_as(first[3])
    finally:
        eng.close()


def test_the_other_calls_do_not_see_it(engine_default):
    """A run-limit admission gives the same reasons and the same cns_get_usage with a release and a charge before and after it."""
    from cranesched_amd import synth
    cluster, jobs, now = synth.make_config("C1")
    tables, lim_jobs = synth.make_limits("C1", cluster, jobs)
    t, js = uc.random_case(3, 300, uc.REL)
    plain, mixed = engine_default(device=0), engine_default(device=0)
    try:
        out = []
        for eng, mix in ((plain, False), (mixed, True)):
            eng.set_nodes(cluster)
            eng.set_run_limits(tables)
            eng.node_select(now, jobs)
            if mix:
                eng.set_usage_tables(t)
                eng.release_usage(js)
            a = eng.apply_run_limits(lim_jobs) + (eng.usage(),)
            if mix:
                eng.charge_usage(js.take(np.flatnonzero(js.user_acct != uc.NONE)), carry=True)
                want, _, _ = up.apply(t, t.state(), uc.REL, js)
                got_nf, got_of, _ = eng.release_usage(js)
                assert eng.usage_tables().differences(want) == []
            b = eng.apply_run_limits(lim_jobs) + (eng.usage(),)
            out.append((a, b))
        for x, y in zip(out[0], out[1]):
            assert np.array_equal(x[0], y[0]) and x[1] == y[1] and x[2].same_as(y[2])
    finally:
        plain.close()
        mixed.close()


def test_input_rules(engine_default):
    t, js = uc.random_case(4, 64, uc.REL)
    eng = engine_default(device=0)
    try:
        with pytest.raises(EngineError) as e:
            eng.release_usage(js)
        assert e.value.status == up.ERR_STATE
        eng.set_usage_tables(t)
        with pytest.raises(EngineError) as e:                      # CARRY before a first apply
            eng.release_usage(js, carry=True)
        assert e.value.status == up.ERR_STATE
        eng.release_usage(js)
        state = eng.usage_tables()
        nf, of, clean = eng.release_usage(js.slice(0, 0), carry=True)     # J == 0 is CNS_OK and writes nothing
        assert len(nf) == 0 and clean == 0 and eng.usage_tables().same_as(state)
        for field, bound in (("user", t.num_users), ("account", t.num_accounts), ("qos", t.num_qos), ("partition", t.num_partitions), ("user_acct", t.num_user_accts)):
            k = js.slice(0, 64)
            getattr(k, field)[9] = bound
            k.skip[9] = 0
            with pytest.raises(EngineError) as e:
                eng.release_usage(k)
            assert e.value.status == up.ERR_INVALID_ARG, field
            k.skip[9] = 1                                          # a skipped row is not read
            eng.release_usage(k)
        k = js.slice(0, 64)
        k.skip[:] = 0
        k.cpu_raw[5] = -1
        with pytest.raises(EngineError) as e:
            eng.release_usage(k)
        assert e.value.status == up.ERR_INVALID_ARG
        k.cpu_raw[5] = 0
        for f in ("cpu_raw", "mem", "wall_sec", "jobs_count", "submit_count", "name_total", "class_count"):
            getattr(k, f)[7] = 0
        with pytest.raises(EngineError) as e:                      # an all-zero delta
            eng.release_usage(k)
        assert e.value.status == up.ERR_INVALID_ARG
        assert eng.usage_tables().same_as(state)                   # refused calls changed nothing
        t.acct_parent[0] = 0                                       # a chain that does not end: a failed set leaves no tables
        with pytest.raises(EngineError) as e:
            eng.set_usage_tables(t)
        assert e.value.status == up.ERR_INVALID_ARG
        with pytest.raises(EngineError) as e:
            eng.release_usage(js)
        assert e.value.status == up.ERR_STATE
    finally:
        eng.close()
