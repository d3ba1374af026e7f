"""A Python model of the device's decomposition of the submit admission (csrc/submit_kernels.inc) and of its bracketing rounds, the exists
bits included, held to tests/submit_pyref.py on seeded cases; and the domino chain, which needs exactly n rounds.

The decomposition: per job at most 8 slots in the reference's order (user, chain accounts, QoS), each with an entity item (exists), a record A
and a record B (submit counts with a threshold), a static code and a code that applies if the entity exists.  One table of integers holds
the five count tables and the exists values; an admission adds to every item of the job.  A round gives every item of an undecided job the
lower value (earlier jobs surely admitted) and the upper value (earlier jobs not surely rejected) it may see; a job that passes under the
upper values is admitted, one that fails under the lower ones is rejected (every check is monotone)."""
import numpy as np
import pytest

from cranesched_amd import abi, submit as sb
from tests import submit_case as sc
from tests import submit_pyref as sp
from tests.limits_pyref import _add_view, _copy_view, _tres_view, _usage_meta

U32 = 0xFFFFFFFF
NOCHECK = U32
C = abi


def decompose(t, jobs, keys):
    """-> per job (pre code, [slot: (stat, ent, keyA, thrA, cond, keyB, thrB)], count, time limit out); table offsets"""
    lay, Q, Pn, U, UA, A = t.layout, t.num_qos, t.num_partitions, t.num_users, t.num_user_accts, t.num_accounts
    base = np.cumsum([0, U * Q, UA * Pn, A * Q, A * Pn, Q, U, A, Q])
    b_uq, b_up, b_aq, b_ap, b_g, e_u, e_a, e_q, NK = (int(x) for x in base)
    view = lambda r: _tres_view(r, lay)
    out = []
    for j in range(jobs.num_jobs):
        tl = int(jobs.time_limit_sec[j])
        count = int(keys.count[j])
        if keys.skip is not None and keys.skip[j]:
            out.append((C.SUBMIT_NOT_CANDIDATE, [], count, tl)); continue
        if count == 0:
            out.append((C.SUBMIT_BAD_COUNT, [], count, tl)); continue
        req = sp._req_total(jobs, lay, j)
        use = sp._times(req, count) if req is not None else None
        if use is None:
            out.append((C.SUBMIT_BAD_REQUEST, [], count, tl)); continue
        q = t.qos[int(keys.qos[j])]
        sjpu, sjpa, sj = int(q["max_submit_jobs_per_user"]), int(q["max_submit_jobs_per_account"]), int(q["max_submit_jobs"])
        pre = 0
        if count > sjpu: pre = C.SUBMIT_MAX_JOB_COUNT_PER_USER
        elif count > sjpa: pre = C.SUBMIT_MAX_JOB_COUNT_PER_ACCOUNT
        elif count > sj: pre = C.SUBMIT_QOS_JOB_COUNT_EXCEEDED
        elif use["cpu"] > int(q["max_cpus_per_user_raw"]): pre = C.SUBMIT_CPUS_PER_TASK_BEYOND
        elif not (sp._ok(use, view(q["max_tres_per_user"])) and sp._ok(use, view(q["max_tres_per_account"])) and sp._ok(use, view(q["max_tres"]))):
            pre = C.SUBMIT_TRES_PER_JOB_BEYOND
        elif tl >= sc.KMAX: tl = int(q["max_time_limit_per_job_sec"])
        elif tl > int(q["max_time_limit_per_job_sec"]): pre = C.SUBMIT_TIME_LIMIT_BEYOND
        if pre:
            out.append((pre, [], count, tl)); continue
        u, x, qi, p = int(keys.user[j]), int(keys.user_acct[j]), int(keys.qos[j]), int(jobs.partition[j])
        deny = bool(q["deny_on_limit"])

        def static_part(li, is_user):
            if li == sb.LIM_NONE:
                return 0, NOCHECK
            lim = t.part_limits[li]
            unl = (sjpu if is_user else sjpa) == U32
            if not sp._ok(req, view(lim["max_tres_per_job"])): return C.SUBMIT_PARTITION_TRES_PER_JOB_BEYOND, NOCHECK
            if int(q["max_time_limit_per_job_sec"]) == sc.KMAX and tl > int(lim["max_wall_duration_per_job_sec"]): return C.SUBMIT_PARTITION_TIME_BEYOND, NOCHECK
            if unl and count > int(lim["max_submit_jobs"]):
                return (C.SUBMIT_PARTITION_MAX_SUBMIT_JOBS_PER_USER if is_user else C.SUBMIT_PARTITION_MAX_SUBMIT_JOBS_PER_ACCOUNT), NOCHECK
            return 0, (int(lim["max_submit_jobs"]) if unl else NOCHECK)

        def cond_entity(tab, i, is_user):
            if not deny:
                return 0
            val = _usage_meta(tab[i], lay) if tab is not None else {"res": {"cpu": 0, "mem": 0, "gres": {}}, "jobs": 0}
            if val["jobs"] + 1 > int(q["max_jobs_per_user" if is_user else "max_jobs_per_account"]):
                return C.SUBMIT_MAX_JOB_COUNT_PER_USER if is_user else C.SUBMIT_MAX_JOB_COUNT_PER_ACCOUNT
            s = _copy_view(req); _add_view(s, val["res"])
            if is_user:
                if s["cpu"] > int(q["max_cpus_per_user_raw"]): return C.SUBMIT_CPUS_PER_TASK_BEYOND
                if not sp._ok(s, view(q["max_tres_per_user"])): return C.SUBMIT_MAX_TRES_PER_USER_BEYOND
            elif not sp._ok(s, view(q["max_tres_per_account"])): return C.SUBMIT_MAX_TRES_PER_ACCOUNT_BEYOND
            return 0

        slots, rejected = [], False
        if x == sb.LIM_NONE:
            slots.append((C.SUBMIT_USER_ACCOUNT_MISMATCH,)); rejected = True
        else:
            s, thr_b = static_part(int(t.user_part_limit[x * Pn + p]) if t.user_part_limit is not None else sb.LIM_NONE, True)
            if s:
                slots.append((s,)); rejected = True
            else:
                slots.append((0, e_u + u, b_uq + u * Q + qi, sjpu, cond_entity(t.user_qos, u * Q + qi, True), b_up + x * Pn + p, thr_b, 0))
        a = int(keys.account[j])
        while a != sb.LIM_NONE and not rejected:
            s, thr_b = static_part(int(t.acct_part_limit[a * Pn + p]) if t.acct_part_limit is not None else sb.LIM_NONE, False)
            if s:
                slots.append((s,)); rejected = True; break
            slots.append((0, e_a + a, b_aq + a * Q + qi, sjpa, cond_entity(t.acct_qos, a * Q + qi, False), b_ap + a * Pn + p, thr_b, 1))
            a = int(t.acct_parent[a])
        if not rejected:
            c = 0
            if deny:
                val = _usage_meta(t.qos_usage[qi], lay) if t.qos_usage is not None else {"res": {"cpu": 0, "mem": 0, "gres": {}}, "jobs": 0, "wall": 0}
                s = _copy_view(req); _add_view(s, val["res"])
                if val["jobs"] + 1 > int(q["max_jobs"]): c = C.SUBMIT_QOS_JOB_COUNT_EXCEEDED
                elif int(q["max_wall_sec"]) > 0 and val["wall"] + tl > int(q["max_wall_sec"]): c = C.SUBMIT_TIME_LIMIT_BEYOND
                elif not sp._ok(s, view(q["max_tres"])): c = C.SUBMIT_TRES_PER_JOB_BEYOND
            slots.append((0, e_q + qi, b_g + qi, sj, c, None, NOCHECK, 2))
        out.append((0, slots, count, tl))
    return out, (b_uq, b_up, b_aq, b_ap, b_g, e_u, e_a, e_q, NK)


CODE_A = (C.SUBMIT_MAX_JOB_COUNT_PER_USER, C.SUBMIT_MAX_JOB_COUNT_PER_ACCOUNT, C.SUBMIT_QOS_JOB_COUNT_EXCEEDED)
CODE_B = (C.SUBMIT_PARTITION_MAX_SUBMIT_JOBS_PER_USER, C.SUBMIT_PARTITION_MAX_SUBMIT_JOBS_PER_ACCOUNT)


def first_failure(slots, count, value):
    """value(key) -> what the item sees"""
    for s in slots:
        if s[0]:
            return s[0]
        _, ent, ka, ta, cond, kb, tb, kind = s
        if value(ent) > 0:
            if ta != NOCHECK and value(ka) + count > ta: return CODE_A[kind]
            if cond: return cond
            if kb is not None and tb != NOCHECK and value(kb) + count > tb: return CODE_B[kind]
    return 0


def items_of(slots, count):
    for s in slots:
        if not s[0]:
            yield s[1], 1
            yield s[2], count
            if s[5] is not None:
                yield s[5], count


def table_of(t, off):
    s = t.state()
    return np.concatenate([s.user_qos_submit, s.user_part_submit, s.acct_qos_submit, s.acct_part_submit, s.qos_submit,
                           s.user_exists, s.acct_exists, s.qos_exists]).astype(np.int64)


def run_rounds(t, jobs, keys, max_rounds=10 ** 9):
    dec, off = decompose(t, jobs, keys)
    st = table_of(t, off)
    J = len(dec)
    code = np.zeros(J, np.uint8)
    state = np.zeros(J, np.uint8)      # 0 undecided, 1 admitted, 2 rejected
    for j, (pre, slots, count, tl) in enumerate(dec):
        if pre or any(s[0] for s in slots):
            state[j] = 2
    rounds = 0
    while (state == 0).any() and rounds < max_rounds:
        rounds += 1
        lo, hi = {}, {}
        new = state.copy()
        for j, (pre, slots, count, tl) in enumerate(dec):   # one sweep in arrival order = the segmented exclusive prefix sums
            if state[j] == 0:
                if first_failure(slots, count, lambda k: st[k] + lo.get(k, 0)): new[j] = 2
                elif not first_failure(slots, count, lambda k: st[k] + hi.get(k, 0)): new[j] = 1
            if not pre:
                for k, add in items_of(slots, count):
                    if state[j] == 1: lo[k] = lo.get(k, 0) + add
                    if state[j] != 2: hi[k] = hi.get(k, 0) + add
        state = new
    if (state == 0).any():
        return None, rounds
    acc = {}
    for j, (pre, slots, count, tl) in enumerate(dec):        # the final pass: exact values
        code[j] = pre or first_failure(slots, count, lambda k: st[k] + acc.get(k, 0))
        assert (code[j] == 0) == (state[j] == 1)
        if code[j] == 0:
            for k, add in items_of(slots, count):
                acc[k] = acc.get(k, 0) + add
    for k, v in acc.items():
        st[k] += v
    return (code, np.array([d[3] for d in dec], np.int64), st), rounds


def flat_state(s):
    return np.concatenate([s.user_qos_submit, s.user_part_submit, s.acct_qos_submit, s.acct_part_submit, s.qos_submit]).astype(np.int64), \
        np.concatenate([s.user_exists, s.acct_exists, s.qos_exists])


def check_against_pyref(t, jobs, keys):
    want = sp.run(t, jobs, keys)
    (code, tlo, st), rounds = run_rounds(t, jobs, keys)
    cnt, ex = flat_state(want[3])
    assert np.array_equal(code, want[0]) and np.array_equal(tlo, want[1])
    assert np.array_equal(st[:len(cnt)], cnt) and np.array_equal(st[len(cnt):] > 0, ex > 0)
    return rounds


def test_hand_table():
    t, jobs, keys = sc.hand_table()[:3]
    check_against_pyref(t, jobs, keys)


@pytest.mark.parametrize("seed", range(12))
def test_seeded_cases(seed):
    worst = 0
    for sub in range(20):                                     # 240 cases in all
        J = [5, 33, 120, 257][sub % 4]
        t, jobs, keys = sc.random_case(seed * 100 + sub, J, U=12, A=10, Q=4, Pn=3, array_frac=0.15)
        worst = max(worst, check_against_pyref(t, jobs, keys))
    print("rounds, worst of 20:", worst)


def test_domino_chain_needs_exactly_n_rounds():
    n = 40
    t, jobs, keys = sc.domino_chain(n)
    want = sp.run(t, jobs, keys)
    (code, tlo, st), rounds = run_rounds(t, jobs, keys)
    assert np.array_equal(code, want[0])
    assert rounds == n
    assert run_rounds(t, jobs, keys, max_rounds=n - 1)[0] is None
