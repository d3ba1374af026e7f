"""Plain-Python restatement of the submit-limit admission, statement by statement, with the reference's line numbers beside each
statement (src/CraneCtld/Accounting/AccountMetaContainer.cpp unless a file is named).  Maps are dicts keyed like the reference's maps;
nothing here shares code with the kernels.  The truth the device results are held to (tests/test_gpu_submit_limits.py); itself held
to a hand-derived table (tests/test_submit_pyref.py)."""
import numpy as np

from cranesched_amd import abi, submit as sb
from tests.limits_pyref import _add_view, _check_tres, _copy_view, _tres_view, _usage_meta

NONE = sb.LIM_NONE
KMAX = abi.SUBMIT_JOB_MAX_TIME_LIMIT_SEC
U32, I64, U64 = (1 << 32) - 1, (1 << 63) - 1, (1 << 64) - 1
ERR_INVALID_ARG, ERR_UNSUPPORTED, ERR_STATE = -1, -4, -5   # cns_status


class Refused(Exception):
    def __init__(self, status):
        super().__init__(status)
        self.status = status


def _req_total(jobs, layout, j):
    """req_total_res_view = req_node_res_view * node_num + req_task_res_view * ntasks (JobScheduler.cpp:7156-7157); None on a 64-bit
    overflow.  GRES lives in the node view only: name totals and class counts x node_num; a zero count is no entry."""
    k, nt = int(jobs.node_num[j]), int(jobs.ntasks[j])
    ncpu = int(jobs.node_cpu_raw[j]) if jobs.node_cpu_raw is not None else 0
    cpu = ncpu * k + int(jobs.task_cpu_raw[j]) * nt
    mem = int(jobs.node_mem[j]) * k + int(jobs.task_mem[j]) * nt
    if not (-I64 - 1 <= ncpu * k <= I64 and -I64 - 1 <= int(jobs.task_cpu_raw[j]) * nt <= I64 and -I64 - 1 <= cpu <= I64 and mem <= U64):
        return None
    gres = {}
    if jobs.gres_total is not None:
        for n in range(abi.MAX_GRES_NAMES):
            if int(jobs.gres_total[j][n]):
                gres[n] = {"total": int(jobs.gres_total[j][n]) * k, "spec": {}}
    if jobs.gres_spec is not None:
        for g in range(len(layout.class_name)):
            if int(jobs.gres_spec[j][g]):
                gres.setdefault(layout.class_name[g], {"total": 0, "spec": {}})["spec"][g] = int(jobs.gres_spec[j][g]) * k
    return {"cpu": cpu, "mem": mem, "gres": gres}


def _times(v, c):                                          # ResourceView operator*(uint32), None on a 64-bit overflow
    r = {"cpu": v["cpu"] * c, "mem": v["mem"] * c,
         "gres": {n: {"total": g["total"] * c, "spec": {t: x * c for t, x in g["spec"].items()}} for n, g in v["gres"].items()}}
    if not -I64 - 1 <= r["cpu"] <= I64 or r["mem"] > U64 or any(g["total"] > U64 or any(x > U64 for x in g["spec"].values()) for g in r["gres"].values()):
        return None
    return r


def _ok(req, total):                                       # CheckTres_ as a bool, :345-360
    return _check_tres(req, total, 0) == 0


def check_inputs(t, jobs, keys, state):
    """The call's input rules (submit_limits.h): raises Refused(status)."""
    J = jobs.num_jobs
    for tab in (t.user_qos, t.user_part, t.acct_qos, t.acct_part, t.qos_usage):
        if tab is not None and len(tab) and int(tab["jobs_count"].max()) == U32:
            raise Refused(ERR_INVALID_ARG)
    total = 0
    for j in range(J):
        if keys.skip is not None and keys.skip[j]:
            continue
        if keys.user[j] >= t.num_users or keys.account[j] >= t.num_accounts or keys.qos[j] >= t.num_qos or jobs.partition[j] >= t.num_partitions \
                or (keys.user_acct[j] != NONE and keys.user_acct[j] >= t.num_user_accts):
            raise Refused(ERR_INVALID_ARG)
        total += int(keys.count[j])
    if state.max_count() + total > U32:
        raise Refused(ERR_UNSUPPORTED)


def run(t, jobs, keys, state=None):
    """-> (code[J] u8, time_limit_out[J] i64, num_admitted, SubmitState after the batch).  t: SubmitTables, jobs: abi.Jobs,
    keys: SubmitKeys; state: the SubmitState to start from (CNS_SUBMIT_CARRY), None = the tables'."""
    lay = t.layout
    Q, Pn = t.num_qos, t.num_partitions
    state = t.state() if state is None else SubmitState_copy(state)
    check_inputs(t, jobs, keys, state)
    qos = [{"sjpu": int(q["max_submit_jobs_per_user"]), "sjpa": int(q["max_submit_jobs_per_account"]), "sj": int(q["max_submit_jobs"]),
            "jpu": int(q["max_jobs_per_user"]), "jpa": int(q["max_jobs_per_account"]), "jobs": int(q["max_jobs"]), "deny": bool(q["deny_on_limit"]),
            "cpu_x": int(q["max_cpus_per_user_raw"]), "wall": int(q["max_wall_sec"]), "tl": int(q["max_time_limit_per_job_sec"]),
            "tres": _tres_view(q["max_tres"], lay), "tpu": _tres_view(q["max_tres_per_user"], lay),
            "tpa": _tres_view(q["max_tres_per_account"], lay)} for q in t.qos]
    plim = [{"sj": int(p["max_submit_jobs"]), "wall": int(p["max_wall_duration_per_job_sec"]), "tres": _tres_view(p["max_tres_per_job"], lay)}
            for p in t.part_limits]
    zero = {"res": {"cpu": 0, "mem": 0, "gres": {}}, "jobs": 0, "wall": 0}

    def meta(tab, i):                                      # jobs_count, resource, wall_time of a record: inputs, as given
        return _usage_meta(tab[i], lay) if tab is not None else zero

    # m_user_meta_map_ / m_account_meta_map_ / m_qos_meta_map_: the entity is in the map or not; its nested submit counts
    users = {u for u in range(t.num_users) if state.user_exists[u]}
    accts = {a for a in range(t.num_accounts) if state.acct_exists[a]}
    qoses = {q for q in range(Q) if state.qos_exists[q]}
    uq, up, aq, ap, qg = state.user_qos_submit, state.user_part_submit, state.acct_qos_submit, state.acct_part_submit, state.qos_submit

    def entity_qos(submit, val, q, is_user, req, count):   # CheckQosSubmitLimitsForEntity_ :374-412 (a missing entry = `empty`, :378-380)
        max_submit = q["sjpu"] if is_user else q["sjpa"]   # :382-383
        if submit + count > max_submit:                    # :384
            return abi.SUBMIT_MAX_JOB_COUNT_PER_USER if is_user else abi.SUBMIT_MAX_JOB_COUNT_PER_ACCOUNT
        if q["deny"]:                                      # :389
            if val["jobs"] + 1 > (q["jpu"] if is_user else q["jpa"]):   # :392
                return abi.SUBMIT_MAX_JOB_COUNT_PER_USER if is_user else abi.SUBMIT_MAX_JOB_COUNT_PER_ACCOUNT
            use = _copy_view(req); _add_view(use, val["res"])           # :397-398
            if is_user:
                if use["cpu"] > q["cpu_x"]:                # :401
                    return abi.SUBMIT_CPUS_PER_TASK_BEYOND
                if not _ok(use, q["tpu"]):                 # :403
                    return abi.SUBMIT_MAX_TRES_PER_USER_BEYOND
            elif not _ok(use, q["tpa"]):                   # :406
                return abi.SUBMIT_MAX_TRES_PER_ACCOUNT_BEYOND
        return 0

    def entity_part(submit, lim, q, is_user, count):       # CheckPartitionSubmitLimitsForEntity_ :414-488
        if lim is None:                                    # :420
            return 0
        if (q["sjpu"] if is_user else q["sjpa"]) != U32:   # :423 / :457
            return 0
        # :432-436 / :467-469; a missing nested entry skips the check, which equals a zero entry: count > max_submit_jobs was
        # tested at :741 / :811 under the same condition
        if submit + count > lim["sj"]:
            return abi.SUBMIT_PARTITION_MAX_SUBMIT_JOBS_PER_USER if is_user else abi.SUBMIT_PARTITION_MAX_SUBMIT_JOBS_PER_ACCOUNT
        return 0

    def static_part(lim, q, is_user, req, tl, count):      # :715-749 / :784-819
        if lim is None:
            return 0
        if not _ok(req, lim["tres"]):                      # :716 / :785
            return abi.SUBMIT_PARTITION_TRES_PER_JOB_BEYOND
        if q["tl"] == KMAX and tl > lim["wall"]:           # :727-728 / :796-797
            return abi.SUBMIT_PARTITION_TIME_BEYOND
        if (q["sjpu"] if is_user else q["sjpa"]) == U32 and count > lim["sj"]:   # :739-741 / :808-811
            return abi.SUBMIT_PARTITION_MAX_SUBMIT_JOBS_PER_USER if is_user else abi.SUBMIT_PARTITION_MAX_SUBMIT_JOBS_PER_ACCOUNT
        return 0

    def check(j):
        """-> (code, time limit after :118-119)"""
        tl = int(jobs.time_limit_sec[j])
        if keys.skip is not None and keys.skip[j]:
            return abi.SUBMIT_NOT_CANDIDATE, tl
        count = int(keys.count[j])
        if count == 0:                                     # JobScheduler.cpp:3466 (:83 would return SUCCESS and add nothing)
            return abi.SUBMIT_BAD_COUNT, tl
        req = _req_total(jobs, lay, j)
        use = _times(req, count) if req is not None else None      # :97
        if use is None:
            return abi.SUBMIT_BAD_REQUEST, tl
        u, x, a0, qi, p = int(keys.user[j]), int(keys.user_acct[j]), int(keys.account[j]), int(keys.qos[j]), int(jobs.partition[j])
        q = qos[qi]
        if count > q["sjpu"]: return abi.SUBMIT_MAX_JOB_COUNT_PER_USER, tl        # :99
        if count > q["sjpa"]: return abi.SUBMIT_MAX_JOB_COUNT_PER_ACCOUNT, tl     # :102
        if count > q["sj"]: return abi.SUBMIT_QOS_JOB_COUNT_EXCEEDED, tl          # :105
        if use["cpu"] > q["cpu_x"]: return abi.SUBMIT_CPUS_PER_TASK_BEYOND, tl    # :108
        if not _ok(use, q["tpu"]) or not _ok(use, q["tpa"]) or not _ok(use, q["tres"]):   # :111-113
            return abi.SUBMIT_TRES_PER_JOB_BEYOND, tl
        if tl >= KMAX:                                     # :118
            tl = q["tl"]                                   # :119
        elif tl > q["tl"]:                                 # :120
            return abi.SUBMIT_TIME_LIMIT_BEYOND, tl
        # ---- CheckSubmitLimits_ :694-889 ----
        if x == NONE:                                      # :702-708
            return abi.SUBMIT_USER_ACCOUNT_MISMATCH, tl
        li = int(t.user_part_limit[x * Pn + p]) if t.user_part_limit is not None else NONE   # :710-713
        ulim = plim[li] if li != NONE else None
        r = static_part(ulim, q, True, req, tl, count)     # :715-749
        if r: return r, tl
        if u in users:                                     # :751 if_contains -> CheckEntitySubmitLimits_ :490-506
            r = entity_qos(int(uq[u * Q + qi]), meta(t.user_qos, u * Q + qi), q, True, req, count) or \
                entity_part(int(up[x * Pn + p]), ulim, q, True, count)
            if r: return r, tl                             # :759-766
        a = a0
        while a != NONE:                                   # :770 job.account_chain, from the job's account to the root
            li = int(t.acct_part_limit[a * Pn + p]) if t.acct_part_limit is not None else NONE   # :779-782
            alim = plim[li] if li != NONE else None
            r = static_part(alim, q, False, req, tl, count)   # :784-819
            if r: return r, tl
            if a in accts:                                 # :821
                r = entity_qos(int(aq[a * Q + qi]), meta(t.acct_qos, a * Q + qi), q, False, req, count) or \
                    entity_part(int(ap[a * Pn + p]), alim, q, False, count)
                if r: return r, tl                         # :829-837
            a = int(t.acct_parent[a])
        if qi in qoses:                                    # :841
            val = meta(t.qos_usage, qi)
            if int(qg[qi]) + count > q["sj"]:              # :844
                return abi.SUBMIT_QOS_JOB_COUNT_EXCEEDED, tl
            if q["deny"]:                                  # :853
                if val["jobs"] + 1 > q["jobs"]:            # :854
                    return abi.SUBMIT_QOS_JOB_COUNT_EXCEEDED, tl
                if q["wall"] > 0 and val["wall"] + tl > q["wall"]:   # :863-864
                    return abi.SUBMIT_TIME_LIMIT_BEYOND, tl
                use = _copy_view(req); _add_view(use, val["res"])    # :875-876
                if not _ok(use, q["tres"]):                # :877
                    return abi.SUBMIT_TRES_PER_JOB_BEYOND, tl
        # ---- MallocMetaSubmitResource :139-153 -> DoMallocResource_ :1067-1124 with submit_jobs_count = count ----
        users.add(u); uq[u * Q + qi] += count; up[x * Pn + p] += count       # :1086-1104
        a = a0
        while a != NONE:                                   # :1106-1116
            accts.add(a); aq[a * Q + qi] += count; ap[a * Pn + p] += count
            a = int(t.acct_parent[a])
        qoses.add(qi); qg[qi] += count                     # :1118-1123
        return abi.SUBMIT_OK, tl

    J = jobs.num_jobs
    code, tlo = np.zeros(J, np.uint8), np.zeros(J, np.int64)
    for j in range(J):
        code[j], tlo[j] = check(j)
    for u in users: state.user_exists[u] = 1
    for a in accts: state.acct_exists[a] = 1
    for q_ in qoses: state.qos_exists[q_] = 1
    return code, tlo, int((code == 0).sum()), state


def SubmitState_copy(s):
    return sb.SubmitState(*[getattr(s, f).copy() for f in sb.SubmitState.__dataclass_fields__])
