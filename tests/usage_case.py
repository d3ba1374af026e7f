"""Inputs for the release / charge tests (include/crane_gpu_usage/usage.h), shared by the CPU tests and the GPU tests: table and row
builders, the named cases at the smallest shapes that can still go wrong, seeded random cases, and the closed form of usage.h written
over plain component vectors (tests/test_usage_pyref.py holds it to the literal fold of tests/usage_pyref.py).

A case is (tables, [(op, rows, carry), ...]): the calls in sequence."""
import numpy as np

from cranesched_amd import abi, usage as us
from cranesched_amd.limits import USAGE_DT

NONE = us.LIM_NONE
REL, CHG = abi.USAGE_RELEASE, abi.USAGE_CHARGE
GIB = 1 << 30
LAYOUT = abi.GresLayout(class_name=[0, 0, 1, 1, 2, 2, 3, 3], class_shift=[0, 8, 16, 24, 32, 40, 48, 56], class_width=[8] * 8)   # two classes per name
COMPONENTS = ["cpu_raw", "mem", "wall_sec", "jobs_count", "submit"] + [f"name{n}" for n in range(4)] + [f"class{g}" for g in range(8)]
U64 = (1 << 64) - 1


def rec(cpu=0, mem=0, wall=0, jobs=0, names=(), classes=()):
    r = np.zeros((), USAGE_DT)
    r["cpu_raw"], r["mem"], r["wall_sec"], r["jobs_count"] = cpu, mem, wall, jobs
    r["name_total"][:len(names)] = names
    r["class_count"][:len(classes)] = classes
    return r


def rec_of_vector(v):
    """17 components in the order of COMPONENTS -> (USAGE_DT record, submit count)."""
    return rec(v[0], v[1], v[2], v[3], v[5:9], v[9:17]), int(v[4])


def tables(parent, U=2, Q=2, Pn=2, value=None, submit=0, layout=LAYOUT, UA=None):
    """Every record exists and holds `value` (a rec()) and `submit`; every entity exists.  The arrays are the caller's to change before
    the tables are handed to the engine."""
    parent = np.asarray(parent, np.uint32)
    A, UA = len(parent), U if UA is None else UA
    value = rec() if value is None else value
    n = {"user_qos": U * Q, "user_part": UA * Pn, "acct_qos": A * Q, "acct_part": A * Pn, "qos_usage": Q}
    kw = {f: np.full(n[f], value, USAGE_DT) for f in us.TABLES}
    kw.update({s: np.full(n[f], submit, np.uint32) for s, f in zip(us.SUBMITS, us.TABLES)})
    kw.update({e: np.ones(n[f], np.uint8) for e, f in zip(us.NESTED, us.TABLES)})
    return us.UsageTables(layout=layout, num_users=U, num_user_accts=UA, num_qos=Q, num_partitions=Pn, acct_parent=parent,
                          user_exists=np.ones(U, np.uint8), acct_exists=np.ones(A, np.uint8), qos_exists=np.ones(Q, np.uint8), **kw)


def rows(*rs):
    """Each row a dict: user, ua (default: user), account, qos, part, cpu, mem, wall, jobs, submit, names, classes, skip."""
    J = len(rs)
    nt, cc = np.zeros((J, 4), np.uint64), np.zeros((J, 8), np.uint64)
    for j, r in enumerate(rs):
        nt[j, :len(r.get("names", ()))] = r.get("names", ())
        cc[j, :len(r.get("classes", ()))] = r.get("classes", ())
    col = lambda k, d=0: [r.get(k, d) for r in rs]
    return us.UsageJobs(col("user"), [r.get("ua", r.get("user", 0)) for r in rs], col("account"), col("qos"), col("part"), col("cpu"), col("mem"),
                        col("wall"), col("jobs"), col("submit"), nt, cc, col("skip"))


def row_of_vector(v, **keys):
    return dict(cpu=int(v[0]), mem=int(v[1]), wall=int(v[2]), jobs=int(v[3]), submit=int(v[4]), names=[int(x) for x in v[5:9]],
                classes=[int(x) for x in v[9:17]], **keys)


FIVE = rec(cpu=5 * 256, mem=5 * GIB, wall=5000, jobs=5, names=(5, 5, 5, 5), classes=(5,) * 8)
ROOT1 = [NONE]
CHAIN6 = [NONE, 0, 1, 2, 3, 4]            # account 5 -> 4 -> 3 -> 2 -> 1 -> 0: a chain of six from 5


# ---- the named cases --------------------------------------------------------------------------------------------------------------------
def one_job():
    return tables(ROOT1, value=FIVE, submit=5), [(REL, rows(dict(cpu=256, mem=GIB, wall=600, jobs=1, submit=1, names=[1], classes=[1])), False)]


def exact_fit():
    """Two jobs on every record with T == val: every nested record is erased, and the second job is clean (nothing is behind it)."""
    half = dict(cpu=512, mem=2 * GIB, wall=2000, jobs=2, submit=2, names=[2, 2, 2, 2], classes=[2] * 8)
    rest = dict(cpu=768, mem=3 * GIB, wall=3000, jobs=3, submit=3, names=[3, 3, 3, 3], classes=[3] * 8)
    return tables(ROOT1, value=FIVE, submit=5), [(REL, rows(half, rest), False)]


def one_over(component):
    """Two jobs, T == val + 1 in exactly one component, T == val in every other."""
    val = np.array([5 * 256, 5 * GIB, 5000, 5, 5] + [5] * 12, dtype=object)
    a = np.array([256, GIB, 1000, 1, 1] + [1] * 12, dtype=object)
    b = val - a
    b[component] += 1
    return tables(ROOT1, value=FIVE, submit=5), [(REL, rows(row_of_vector(a), row_of_vector(b)), False)]


def middle_trips(order=(0, 1, 2)):
    """Three jobs on every record: 2 + 4 > 5 in jobs_count, so in the order (0, 1, 2) the middle one over-frees and the last finds the keys
    gone; 2 + 1 fits, so in the order (0, 2, 1) the last one over-frees.  The tables end at zero either way."""
    js = [dict(jobs=2, cpu=256), dict(jobs=4, cpu=256), dict(jobs=1, cpu=256)]
    return tables(ROOT1, value=FIVE, submit=5), [(REL, rows(*[js[i] for i in order]), False)]


def qos_over_freed_twice():
    """Only the QoS entity exists: its global record is never erased, every job behind the first over-free over-frees again."""
    t = tables(ROOT1, value=FIVE, submit=5)
    t.user_exists[:] = 0
    t.acct_exists[:] = 0
    return t, [(REL, rows(dict(jobs=3), dict(jobs=3), dict(jobs=1), dict(submit=1)), False)]


def class_the_record_lacks():
    t = tables(ROOT1, value=rec(cpu=1024, mem=4 * GIB, wall=100, jobs=4, names=(4,), classes=(4, 0)), submit=0)
    return t, [(REL, rows(dict(cpu=256, jobs=1, names=[1], classes=[0, 1]), dict(cpu=256, jobs=1, names=[1], classes=[1])), False)]


def absent_user_entity():
    """User 0 has no record but its nested values are non-zero: untouched, no bits; the accounts and the QoS are released."""
    t = tables(ROOT1, value=FIVE, submit=5)
    t.user_exists[0] = 0
    return t, [(REL, rows(dict(user=0, jobs=1, cpu=256), dict(user=1, jobs=1, cpu=256)), False)]


def user_acct_none():
    return tables(ROOT1, value=FIVE, submit=5), [(REL, rows(dict(user=1, ua=NONE, jobs=1), dict(user=1, ua=1, jobs=1)), False)]


def chain(length):
    parent = CHAIN6[:length]
    t = tables(parent, value=FIVE, submit=5)
    t.acct_exists[length // 2] = 0                    # an account in the middle of the chain without a record (the root for a chain of 1 ... 2)
    js = [dict(account=length - 1, jobs=2, cpu=256, wall=10), dict(account=length - 1, jobs=2, submit=5), dict(account=length - 1, jobs=2)]
    return t, [(REL, rows(*js), False)]


def one_record(J, seed=0, exact=False):
    """Only the QoS entity exists: every job touches the one global record, J items in one segment.  The record holds what the first
    trip_at jobs free (exact) or one unit less, so the fold trips deep inside the segment."""
    r = np.random.default_rng(seed)
    t = tables(ROOT1, U=1, Q=1, Pn=1)
    t.user_exists[:] = 0
    t.acct_exists[:] = 0
    v = r.integers(0, 4, (J, 17))
    v[:, 3] = 1
    trip_at = (2 * J) // 3
    tot = v[:trip_at].sum(axis=0)
    if not exact:
        tot[1] -= 1 if tot[1] else 0
        tot[3] -= 1
    t.qos_usage[0], t.qos_submit[0] = rec_of_vector(tot)
    return t, [(REL, rows(*[row_of_vector(v[j]) for j in range(J)]), False)]


def one_nested_record(J, seed=0):
    """One user and nothing else: every job touches the one (user, qos) record; user_acct == NONE.  The record holds exactly what the
    first 2J/3 jobs free: it is erased there and every job behind finds the key gone."""
    r = np.random.default_rng(seed)
    t = tables(ROOT1, U=1, Q=1, Pn=1)
    t.acct_exists[:] = 0
    t.qos_exists[:] = 0
    v = r.integers(0, 4, (J, 17))
    v[:, 4] = 1
    t.user_qos[0], t.user_qos_submit[0] = rec_of_vector(v[:(2 * J) // 3].sum(axis=0))
    return t, [(REL, rows(*[row_of_vector(v[j], ua=NONE) for j in range(J)]), False)]


def own_records(J):
    """Every job on records of its own: its own user, user_acct and root account; the shared QoS has no record."""
    t = tables([NONE] * J, U=J, Q=1, Pn=1, value=rec(cpu=512, jobs=2), submit=1)
    t.qos_exists[:] = 0
    return t, [(REL, rows(*[dict(user=j, account=j, cpu=256 * (1 + j % 3), jobs=1 + j % 2, submit=j % 2) for j in range(J)]), False)]


def saturating_prefix():
    """mem: the record holds UINT64_MAX, two jobs free 2^63 each: the prefix leaves 64 bits, which fits nothing, not even UINT64_MAX."""
    t = tables(ROOT1, value=rec(mem=U64, jobs=9), submit=0)
    return t, [(REL, rows(dict(mem=1 << 63, jobs=1), dict(mem=1 << 63, jobs=1), dict(mem=5, jobs=1)), False)]


def charge_creates():
    """Nothing exists; two charges create user 1, the accounts of the chain 2 -> 1 -> 0, QoS 1 and their nested records."""
    t = us.UsageTables(layout=LAYOUT, num_users=2, num_user_accts=2, num_qos=2, num_partitions=2, acct_parent=np.array([NONE, 0, 1], np.uint32))
    js = [dict(user=1, account=2, qos=1, part=1, cpu=512, mem=GIB, wall=3600, jobs=1, submit=1, names=[2], classes=[1, 1]),
          dict(user=1, account=2, qos=1, part=0, submit=7)]
    return t, [(CHG, rows(*js), False)]


def charge_wraps():
    """A release that succeeds, then a charge that takes a submit count to 2^32: refused, the tables stay as the release left them."""
    t = tables(ROOT1, value=FIVE, submit=0xFFFFFFFE)
    return t, [(REL, rows(dict(jobs=1)), False), (CHG, rows(dict(submit=1), dict(submit=1)), True), (CHG, rows(dict(submit=1), dict(submit=1)), False),
               (CHG, rows(dict(submit=1)), True)]


def carry_sequence(seed=3):
    t, a = random_case(seed, 150, REL)
    _, b = random_case(seed + 1, 150, CHG)
    _, c = random_case(seed + 2, 150, REL)
    return t, [(REL, a, False), (CHG, b, True), (REL, c, True), (REL, c, False)]


def random_tables(seed, U=6, A=7, Q=2, Pn=2, hi=40, parent=None, present=0.8, lo=0, zeros=0.2, nested=0.85):
    r = np.random.default_rng(seed)
    if parent is None:
        parent = np.full(A, NONE, np.uint32)
        depth = np.ones(A, np.int64)
        for a in range(2, A):
            p = int(r.integers(0, a))
            while depth[p] >= 6:
                p = int(r.integers(0, a))
            parent[a], depth[a] = p, depth[p] + 1
    A = len(parent)
    t = tables(parent, U=U, Q=Q, Pn=Pn)
    for f, s, e in zip(us.TABLES, us.SUBMITS, us.NESTED + (None,)):
        n = len(getattr(t, f))
        v = r.integers(lo, hi, (n, 17))
        v[r.random((n, 17)) < zeros] = 0
        for i in range(n):
            getattr(t, f)[i], getattr(t, s)[i] = rec_of_vector(v[i])
        if e:
            getattr(t, e)[:] = r.random(n) < nested
    t.user_exists[:] = r.random(U) < present
    t.acct_exists[:] = r.random(A) < present
    t.qos_exists[:] = r.random(Q) < present
    return t


def random_case(seed, J, op, account=None, **kw):
    """A few entities, a few hundred jobs: every record is contested.  account: every job's account (else random)."""
    t = random_tables(seed, **kw)
    r = np.random.default_rng(seed + 1000)
    v = r.integers(0, 4, (J, 17))
    v[r.random((J, 17)) < 0.5] = 0
    v[:, 3] = np.maximum(v[:, 3], (v.sum(axis=1) == 0))      # no all-zero delta
    user = r.integers(0, t.num_users, J)
    ua = np.where(r.random(J) < 0.05, NONE, user) if op == REL else user
    js = rows(*[row_of_vector(v[j], user=int(user[j]), ua=int(ua[j]), account=int(r.integers(0, t.num_accounts)) if account is None else account, qos=int(r.integers(0, t.num_qos)),
                              part=int(r.integers(0, t.num_partitions)), skip=int(r.random() < 0.03)) for j in range(J)])
    return t, js


def deep_contested(J, seed=11):
    """Every entity exists and every job sits at the bottom of the chain of six: exactly 15 items per job, the account records shared by
    all of them.  A delta component averages 0.75 and every record component lies in [J / 4, J / 2): the shared records trip between a
    third and two thirds of the way through the call, the users' records (J / 16 jobs each) never."""
    return random_case(seed, J, REL, account=5, U=8, Q=2, Pn=2, lo=J // 4, hi=J // 2, zeros=0.0, parent=np.array(CHAIN6, np.uint32), present=1.1, nested=1.1)


# ---- the closed form of usage.h over component vectors ---------------------------------------------------------------------------------
CLEAN, OVER_FREE, NOT_FOUND = 0, 1, 2


def closed_form(val, exists, deltas, nested):
    """val: the record's components (None-free ints), exists: the nested record's byte (ignored for the QoS record), deltas: the jobs'
    component vectors in call order.  -> (final components, exists after, per-job status)."""
    n = len(val)
    if nested and not exists:
        return list(val), 0, [NOT_FOUND] * len(deltas)
    fits = lambda p: all(p[c] <= val[c] for c in range(n))
    status, prefix = [], [0] * n
    for k, d in enumerate(deltas):
        before = list(prefix)
        prefix = [prefix[c] + d[c] for c in range(n)]
        if fits(prefix):
            status.append(CLEAN)
        elif k == 0 or not nested or (fits(before) and before != list(val)):
            status.append(OVER_FREE)
        else:
            status.append(NOT_FOUND)
    final = [val[c] - prefix[c] for c in range(n)] if fits(prefix) else [0] * n
    return final, (1 if any(final) else 0) if nested else 1, status
