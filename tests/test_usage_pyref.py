"""tests/usage_pyref.py (the literal restatement of DoFreeResource_ / DoMallocResource_) held to answers derived by hand from the cited
lines for each of the reference's callers, and the closed form of include/crane_gpu_usage/usage.h (tests/usage_case.closed_form: final
values from the total, masks from the prefix sums) held to that literal fold on random small records, with and without the erase.
No GPU, no engine."""
import copy

import numpy as np

from cranesched_amd import abi
from tests import usage_case as uc
from tests import usage_pyref as up

NONE = up.NONE


def _container():
    """user "u" (0) with account "a" (user_acct 0), chain a (1) -> root (0), QoS 0, partition 0; every record holds the same."""
    val = lambda: up.meta(up.view(1024, 8 * uc.GIB, {0: {"total": 2, "spec": {0: 2}}}), jobs=2, submit=3, wall=7200)
    return {"user": {0: {"qos": {0: val()}, "acct": {0: {0: val()}}}},
            "account": {1: {"qos": {0: val()}, "part": {0: val()}}, 0: {"qos": {0: val()}, "part": {0: val()}}},
            "qos": {0: val()}}


ALLOC = up.view(512, 4 * uc.GIB, {0: {"total": 1, "spec": {0: 1}}})


def _every_record(m):
    return [m["user"][0]["qos"].get(0), m["user"][0]["acct"][0].get(0), m["account"][1]["qos"].get(0), m["account"][1]["part"].get(0),
            m["account"][0]["qos"].get(0), m["account"][0]["part"].get(0), m["qos"].get(0)]


def test_free_meta_resource_of_a_job_in_ctld():
    """:243-254: {alloc, 1, child ? 0 : 1, time_limit}: 1024 - 512 cpu, 8 - 4 GiB, gres 2 - 1, jobs 2 - 1, submit 3 - 1 (3 - 0 for a child),
    wall 7200 - 3600, on all seven records."""
    for child, submit in ((False, 2), (True, 3)):
        m = _container()
        assert up.do_free(m, 0, 0, [1, 0], 0, 0, up.free_meta_resource_ctld(ALLOC, 3600, child)) == (0, 0)
        want = up.meta(up.view(512, 4 * uc.GIB, {0: {"total": 1, "spec": {0: 1}}}), jobs=1, submit=submit, wall=3600)
        assert _every_record(m) == [want] * 7


def test_free_meta_running_resource_and_the_pending_job_form():
    """:256-269 and :271-283: {alloc, 1, 0, time_limit}: the submit count stays."""
    for delta in (up.free_meta_running_resource(ALLOC, 3600), up.free_meta_resource_pd(ALLOC, 3600)):
        m = _container()
        assert up.do_free(m, 0, 0, [1, 0], 0, 0, delta) == (0, 0)
        assert _every_record(m) == [up.meta(up.view(512, 4 * uc.GIB, {0: {"total": 1, "spec": {0: 1}}}), jobs=1, submit=3, wall=3600)] * 7


def test_free_meta_submit_resource():
    """:226-241: {0, 0, count, 0}.  count 3 leaves submit 0 but the records stay (the rest is non-zero); count 4 > 3 zeroes every record
    (:1157), erases the six nested ones (:1159) and keeps the QoS record, zero (:1200)."""
    m = _container()
    assert up.do_free(m, 0, 0, [1, 0], 0, 0, up.free_meta_submit_resource(3)) == (0, 0)
    assert [r["submit"] for r in _every_record(m)] == [0] * 7 and [r["jobs"] for r in _every_record(m)] == [2] * 7
    m = _container()
    every = sum(1 << b for b in (0, 1, 2, 3, 4, 5, 14))
    assert up.do_free(m, 0, 0, [1, 0], 0, 0, up.free_meta_submit_resource(4)) == (0, every)
    assert _every_record(m) == [None] * 6 + [up.meta()]
    # the job behind it: the six keys are gone (:1143), the QoS record over-frees again (:1196)
    assert up.do_free(m, 0, 0, [1, 0], 0, 0, up.free_meta_submit_resource(1)) == (every & ~(1 << 14), 1 << 14)


def test_exact_free_erases_and_the_next_job_finds_nothing():
    m = _container()
    whole = up.meta(up.view(1024, 8 * uc.GIB, {0: {"total": 2, "spec": {0: 2}}}), jobs=2, submit=3, wall=7200)
    assert up.do_free(m, 0, 0, [1, 0], 0, 0, whole) == (0, 0)
    assert _every_record(m) == [None] * 6 + [up.meta()]
    nested = sum(1 << b for b in (0, 1, 2, 3, 4, 5))
    assert up.do_free(m, 0, 0, [1, 0], 0, 0, up.free_meta_submit_resource(1)) == (nested, 1 << 14)


def test_missing_entities_and_the_missing_account_map():
    m = _container()
    del m["user"][0]                     # :1162: nothing under the user, no message
    del m["account"][1]                  # :1180
    assert up.do_free(m, 0, 0, [1, 0], 0, 0, up.free_meta_submit_resource(1)) == (0, 0)
    assert m["account"][0]["qos"][0]["submit"] == 2 and m["qos"][0]["submit"] == 2
    m = _container()
    assert up.do_free(m, 0, NONE, [1, 0], 0, 0, up.free_meta_submit_resource(1)) == (1 << 1, 0)      # :1172
    assert m["user"][0]["acct"][0][0]["submit"] == 3 and m["user"][0]["qos"][0]["submit"] == 2
    del m["qos"][0]                      # :1190
    assert up.do_free(m, 0, 0, [0], 0, 0, up.free_meta_submit_resource(1)) == (0, 0)
    # a GRES class the record lacks (PH:63-64): the whole record is zeroed, not only the class
    m = _container()
    d = up.meta(up.view(0, 0, {0: {"total": 1, "spec": {1: 1}}}), jobs=1)
    assert up.do_free(m, 0, 0, [], 0, 0, d) == (0, 1 | 2 | 1 << 14)


def test_the_two_recovery_charges():
    """:139-153 {0, 0, count, 0} and :155-178 {alloc, 1, child ? 0 : 1, time_limit} through DoMallocResource_: += where the key exists,
    the delta itself where it does not, entities created."""
    m = {"user": {}, "account": {}, "qos": {}}
    up.do_malloc(m, 0, 0, [1, 0], 0, 0, up.malloc_meta_submit_resource(5))
    assert _every_record(m) == [up.meta(submit=5)] * 7
    up.do_malloc(m, 0, 0, [1, 0], 0, 0, up.malloc_recovered_running(ALLOC, 3600, False))
    assert _every_record(m) == [up.meta(copy.deepcopy(ALLOC), jobs=1, submit=6, wall=3600)] * 7
    up.do_malloc(m, 0, 0, [1, 0], 0, 1, up.malloc_recovered_running(ALLOC, 60, True))      # another partition: new nested entries, submit 0
    assert m["user"][0]["acct"][0][1] == m["account"][0]["part"][1] == up.meta(copy.deepcopy(ALLOC), jobs=1, submit=0, wall=60)
    assert m["qos"][0] == up.meta(up.view(1024, 8 * uc.GIB, {0: {"total": 2, "spec": {0: 2}}}), jobs=2, submit=6, wall=3660)


def _vec_meta(v):
    """(cpu, mem, wall, jobs, submit, name 0 total, class 0, class 1) -> a MetaResource; zero counts are no entries."""
    gres = {}
    if v[5] or v[6] or v[7]:
        gres[0] = {"total": v[5], "spec": {t: c for t, c in ((0, v[6]), (1, v[7])) if c}}
    return up.meta(up.view(v[0], v[1], gres), v[3], v[4], v[2])


def _meta_vec(m):
    if m is None:
        return [0] * 8
    g = m["res"]["gres"].get(0, {"total": 0, "spec": {}})
    return [m["res"]["cpu"], m["res"]["mem"], m["wall"], m["jobs"], m["submit"], g["total"], g["spec"].get(0, 0), g["spec"].get(1, 0)]


def test_closed_form_against_the_literal_fold():
    """120 000 random records of 8 small components with 1 - 5 jobs each: the nested (user, qos) record (erased at zero) and the global QoS
    record (never erased) start from the same value and see the same jobs; final values and per-job status from the closed form equal the
    literal fold.  Small ranges make exact fits, ties and trips in every position frequent; the counts below say how frequent."""
    r = np.random.default_rng(20)
    N = 120_000
    seen = {"exact": 0, "trip": 0, "behind_exact": 0, "clean": 0}
    vals, njobs, deltas = r.integers(0, 6, (N, 8)), r.integers(1, 6, N), r.integers(0, 3, (N, 5, 8))
    sparse = r.random((N, 5, 8)) < 0.45
    for i in range(N):
        val = [int(x) for x in vals[i]]
        ds = []
        for k in range(int(njobs[i])):
            d = [0 if sparse[i, k, c] else int(deltas[i, k, c]) for c in range(8)]
            if not any(d):
                d[3] = 1                                        # the caller sends no all-zero delta
            ds.append(d)
        if i % 3 == 0:                                          # a third of the records hold exactly what their first k jobs free
            k = 1 + int(vals[i][0]) % len(ds)
            val = [sum(d[c] for d in ds[:k]) for c in range(8)]
        exists = any(val) or i % 7 == 0                         # now and then a zero record that exists
        m = {"user": {0: {"qos": {0: _vec_meta(val)} if exists else {}, "acct": {}}}, "account": {}, "qos": {0: _vec_meta(val)}}
        got_n, got_q = [], []
        for d in ds:
            nf, of = up.do_free(m, 0, NONE, [], 0, 0, _vec_meta(d))
            got_n.append(uc.NOT_FOUND if nf & 1 else uc.OVER_FREE if of & 1 else uc.CLEAN)
            got_q.append(uc.OVER_FREE if of >> 14 & 1 else uc.CLEAN)
            assert not nf >> 14 & 1
        fin_n, ex_n, st_n = uc.closed_form(val, 1 if exists else 0, ds, nested=True)
        fin_q, _, st_q = uc.closed_form(val, 1, ds, nested=False)
        assert st_n == got_n and st_q == got_q, (val, ds)
        assert (0 in m["user"][0]["qos"]) == bool(ex_n), (val, ds)
        assert _meta_vec(m["user"][0]["qos"].get(0)) == (fin_n if ex_n else [0] * 8), (val, ds)
        assert _meta_vec(m["qos"][0]) == fin_q, (val, ds)
        seen["exact"] += exists and not ex_n and uc.OVER_FREE not in st_n
        seen["trip"] += uc.OVER_FREE in st_n
        seen["behind_exact"] += uc.NOT_FOUND in st_n and uc.OVER_FREE not in st_n and exists
        seen["clean"] += set(st_n) == {uc.CLEAN}
    assert min(seen.values()) > 500, seen


def test_missing_nested_entry_equals_zero_entry_on_the_values():
    """A nested record that does not exist and one that exists holding zero end with the same table values (zero, not existing) under
    any release; only the message differs (key gone / freed more than allocated)."""
    t, js = uc.random_case(5, 60, uc.REL)
    for e in up.us.NESTED:
        getattr(t, e)[::3] = 0
    s0 = t.state()
    a, nf_a, of_a = up.apply(t, s0, uc.REL, js)
    s1 = t.state()
    for e in up.us.NESTED:
        getattr(s1, e)[:] = 1                                   # the same values (zero where it did not exist), every entry present
    b, nf_b, of_b = up.apply(t, s1, uc.REL, js)
    assert [f for f in a.differences(b) if not f.endswith("_exists")] == []
    assert np.array_equal(nf_a | of_a, nf_b | of_b) and not np.array_equal(nf_a, nf_b)
    for e in up.us.NESTED:                                      # what was missing stays missing; as a zero entry it is erased once touched
        assert not getattr(a, e)[::3].any()


def test_dense_and_maps_round_trip_and_bits():
    t = uc.random_tables(9)
    s = t.state()
    assert up.from_maps(up.to_maps(s, t), t).differences(s) == []
    assert abi.usage_bit_acct_qos(5) == 12 and abi.usage_bit_acct_part(5) == 13 and abi.USAGE_BIT_QOS == 14 and abi.USAGE_SLOTS == 15
