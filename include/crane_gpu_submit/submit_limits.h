/*
 * crane_gpu_submit/submit_limits.h — is each submission of a batch ADMITTED by the submit limits of its user, its accounts and its QoS?
 * (A directory of its own beside crane_gpu/, as crane_gpu_probe/, crane_gpu_resv/, crane_gpu_valid/ and crane_gpu_commit/: that
 * directory's file list is the pinned ABI 4 surface, tests/test_abi.py; this header adds calls and changes no existing struct, so
 * CNS_ABI_VERSION stays 4.)
 *
 * Reference (paths relative to the CraneSched tree):
 *   call site, JobScheduler::SubmitJobToScheduler            src/CraneCtld/JobScheduler.cpp:3465-3476 (behind CheckJobValidity, :3458)
 *   AccountMetaContainer::TryMallocMetaSubmitResource        src/CraneCtld/Accounting/AccountMetaContainer.cpp:75-137
 *   MallocMetaSubmitResource -> DoMallocResource_            :139-153, :1067-1124
 *   CheckSubmitLimits_ (user -> account chain -> global QoS) :694-889
 *   CheckQosSubmitLimitsForEntity_ / CheckPartitionSubmitLimitsForEntity_ / CheckEntitySubmitLimits_   :374-506
 *   CheckTres_ / CheckGres_                                  :345-360, :1030-1050
 *
 * What it computes: for J submissions IN THE ORDER GIVEN (arrival order) TryMallocMetaSubmitResource(job, user, count) followed by
 * MallocMetaSubmitResource, statement by statement: job i sees the counters as jobs 0..i-1 left them.  code[j] is the FIRST failing
 * check in the reference's order (all integers, no tolerance):
 *    1. skip[j] != 0                                           CNS_SUBMIT_NOT_CANDIDATE   nothing is read or added
 *    2. count == 0                                             CNS_SUBMIT_BAD_COUNT       the caller's :3466
 *    3. a 64-bit overflow in req_total = node*node_num + task*ntasks (JobScheduler.cpp:7156-7157: cpu, mem; GRES name totals and class
 *       counts x node_num) or in req_total*count               CNS_SUBMIT_BAD_REQUEST
 *    4. :99  count > max_submit_jobs_per_user                  CNS_SUBMIT_MAX_JOB_COUNT_PER_USER
 *    5. :102 count > max_submit_jobs_per_account               CNS_SUBMIT_MAX_JOB_COUNT_PER_ACCOUNT
 *    6. :105 count > max_submit_jobs                           CNS_SUBMIT_QOS_JOB_COUNT_EXCEEDED
 *    7. :108 (req_total*count).cpu > max_cpus_per_user         CNS_SUBMIT_CPUS_PER_TASK_BEYOND
 *    8. :111-114 CheckTres_(req_total*count, max_tres_per_user / max_tres_per_account / max_tres)   CNS_SUBMIT_TRES_PER_JOB_BEYOND
 *    9. :118-123 time_limit >= CNS_SUBMIT_JOB_MAX_TIME_LIMIT_SEC: time_limit = max_time_limit_per_job (the later checks read the new
 *       value); else time_limit > max_time_limit_per_job       CNS_SUBMIT_TIME_LIMIT_BEYOND
 *   10. user entity, static part (:701-749): user_acct == CNS_LIM_NONE              CNS_SUBMIT_USER_ACCOUNT_MISMATCH
 *       with a limit record of (user_acct, partition):
 *         CheckTres_(req_total, max_tres_per_job)                                   CNS_SUBMIT_PARTITION_TRES_PER_JOB_BEYOND
 *         the QoS's max_time_limit_per_job == CNS_SUBMIT_JOB_MAX_TIME_LIMIT_SEC and time_limit > max_wall_duration_per_job
 *                                                                                   CNS_SUBMIT_PARTITION_TIME_BEYOND
 *         max_submit_jobs_per_user == UINT32_MAX and count > max_submit_jobs        CNS_SUBMIT_PARTITION_MAX_SUBMIT_JOBS_PER_USER
 *   11. user entity, ONLY IF THE USER'S RECORD EXISTS (if_contains, :751):
 *         :384 submit(user, qos) + count > max_submit_jobs_per_user                 CNS_SUBMIT_MAX_JOB_COUNT_PER_USER
 *         with deny_on_limit: :392 jobs_count + 1 > max_jobs_per_user               the same code
 *                             :401 (req_total + usage).cpu > max_cpus_per_user      CNS_SUBMIT_CPUS_PER_TASK_BEYOND
 *                             :403 CheckTres_(req_total + usage, max_tres_per_user) CNS_SUBMIT_MAX_TRES_PER_USER_BEYOND (x 1, not x count)
 *         :422-445 under 10's last condition: submit(user_acct, partition) + count > max_submit_jobs
 *                                                                                   CNS_SUBMIT_PARTITION_MAX_SUBMIT_JOBS_PER_USER
 *   12. every account of the chain, from the job's account to the root: the static part (:771-819, as 10 with the account's limit record
 *       and max_submit_jobs_per_account: ..._PER_ACCOUNT), then ONLY IF THE ACCOUNT'S RECORD EXISTS :821-837 as 11 with the per-account
 *       limits: CNS_SUBMIT_MAX_JOB_COUNT_PER_ACCOUNT, CNS_SUBMIT_MAX_TRES_PER_ACCOUNT_BEYOND, CNS_SUBMIT_PARTITION_MAX_SUBMIT_JOBS_PER_ACCOUNT
 *   13. global QoS, ONLY IF THE QOS RECORD EXISTS (:841-886): submit + count > max_submit_jobs   CNS_SUBMIT_QOS_JOB_COUNT_EXCEEDED
 *         with deny_on_limit: jobs_count + 1 > max_jobs                             the same code
 *                             max_wall > 0 and wall + time_limit > max_wall         CNS_SUBMIT_TIME_LIMIT_BEYOND
 *                             CheckTres_(req_total + usage, max_tres)               CNS_SUBMIT_TRES_PER_JOB_BEYOND
 *   14. otherwise CNS_SUBMIT_OK: `count` is added to submit_jobs_count of (user, qos), (user_acct, partition), (account, qos) and
 *       (account, partition) of every chain account and of the QoS, and the user's, every chain account's and the QoS's record is
 *       CREATED if it was absent (:1086-1123) — which switches on 11 - 13 for the jobs behind it.
 * time_limit_out[j] = the time limit after step 9 (the input value for a job that stops before step 9).
 *
 * Canonical model: dense indices, cns_tres, cns_usage and CheckGres_'s canonical walk are those of crane_gpu/run_limits.h.  During a
 * batch only submit_jobs_count of the five record tables and one EXISTS bit per user, account and QoS change; jobs_count, resource and
 * wall_time are inputs.  A missing nested entry (the QoS map or the partition map of an entity) equals a zero entry: :378-380
 * substitutes an empty record, and the check :436 / :469 skips equals the static check :741 / :811 made under the same condition.
 * Entity existence is not equivalent to zero and is carried.  A sum of usage and request beyond 64 bits counts as beyond the limit.
 *
 * Input rules.  CNS_ERR_STATE before cns_set_submit_limits.  CNS_ERR_INVALID_ARG: a missing array; user / account / qos / partition of a
 * job that is not skipped out of range; user_acct neither CNS_LIM_NONE nor in range; a jobs_count of UINT32_MAX; an account chain that
 * does not end.  CNS_ERR_UNSUPPORTED: a chain of more than CNS_LIM_MAX_CHAIN accounts; more than CNS_SUBMIT_MAX_JOBS jobs in one call;
 * max(submit count over all records) + the sum of `count` over the call's jobs that are not skipped > UINT32_MAX (the reference adds the
 * partition and global counts in 32 bits, :436, :469, :844: within the rule no sum wraps).  num_jobs == 0 is CNS_OK and writes nothing.
 * Never a device fault; no kernel of the call waits for another workgroup.  Single device only (not served through cns_group_*).  The
 * call reads and writes device buffers of its own: a cycle, cns_validate_jobs or cns_apply_run_limits before or after it behaves exactly
 * as without it.  Ownership, errors, threading: as in node_select.h.  There is no CPU fallback.
 *
 * With the caller: the uid / user / account lookups and the partition permission (:3400-3456), UserAddJob and job.qos_priority (:116).
 * The frees (FreeMetaSubmitResource) when a job leaves the queue are cns_usage_apply, ../crane_gpu_usage/usage.h.
 */
#ifndef CRANE_GPU_SUBMIT_LIMITS_H_
#define CRANE_GPU_SUBMIT_LIMITS_H_

#include <stdint.h>

#include "../crane_gpu/run_limits.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CNS_SUBMIT_JOB_MAX_TIME_LIMIT_SEC INT64_C(315576000000) /* kJobMaxTimeLimitSec, CtldPublicDefs.h */
#define CNS_SUBMIT_CARRY 1u                                      /* flags: start from what the previous call left */
#define CNS_SUBMIT_MAX_JOBS 16777216u                            /* jobs of one call */

typedef enum cns_submit_code {
  CNS_SUBMIT_OK = 0,
  CNS_SUBMIT_NOT_CANDIDATE = 1,
  CNS_SUBMIT_BAD_COUNT = 2,
  CNS_SUBMIT_BAD_REQUEST = 3,
  CNS_SUBMIT_MAX_JOB_COUNT_PER_USER = 4,                 /* ERR_MAX_JOB_COUNT_PER_USER                */
  CNS_SUBMIT_MAX_JOB_COUNT_PER_ACCOUNT = 5,              /* ERR_MAX_JOB_COUNT_PER_ACCOUNT             */
  CNS_SUBMIT_QOS_JOB_COUNT_EXCEEDED = 6,                 /* ERR_QOS_JOB_COUNT_EXCEEDED                */
  CNS_SUBMIT_CPUS_PER_TASK_BEYOND = 7,                   /* ERR_CPUS_PER_TASK_BEYOND                  */
  CNS_SUBMIT_TRES_PER_JOB_BEYOND = 8,                    /* ERR_TRES_PER_JOB_BEYOND                   */
  CNS_SUBMIT_TIME_LIMIT_BEYOND = 9,                      /* ERR_TIME_TIMIT_BEYOND                     */
  CNS_SUBMIT_USER_ACCOUNT_MISMATCH = 10,                 /* ERR_USER_ACCOUNT_MISMATCH                 */
  CNS_SUBMIT_PARTITION_TRES_PER_JOB_BEYOND = 11,         /* ERR_PARTITION_TRES_PER_JOB_BEYOND         */
  CNS_SUBMIT_PARTITION_TIME_BEYOND = 12,                 /* ERR_PARTITION_TIME_BEYOND                 */
  CNS_SUBMIT_PARTITION_MAX_SUBMIT_JOBS_PER_USER = 13,    /* ERR_PARTITION_MAX_SUBMIT_JOBS_PER_USER    */
  CNS_SUBMIT_PARTITION_MAX_SUBMIT_JOBS_PER_ACCOUNT = 14, /* ERR_PARTITION_MAX_SUBMIT_JOBS_PER_ACCOUNT */
  CNS_SUBMIT_MAX_TRES_PER_USER_BEYOND = 15,              /* ERR_MAX_TRES_PER_USER_BEYOND              */
  CNS_SUBMIT_MAX_TRES_PER_ACCOUNT_BEYOND = 16            /* ERR_MAX_TRES_PER_ACCOUNT_BEYOND           */
} cns_submit_code;

/* The fields of Qos the submit checks read (AccountDefs.h:27-49). */
typedef struct cns_submit_qos {
  uint32_t max_submit_jobs_per_user;
  uint32_t max_submit_jobs_per_account;
  uint32_t max_submit_jobs;
  uint32_t max_jobs_per_user;
  uint32_t max_jobs_per_account;
  uint32_t max_jobs;
  uint32_t deny_on_limit;               /* flags[QosFlags::DenyOnLimit] */
  uint32_t reserved0;
  int64_t max_cpus_per_user_raw;
  int64_t max_wall_sec;                 /* 0 = unlimited */
  int64_t max_time_limit_per_job_sec;
  cns_tres max_tres;
  cns_tres max_tres_per_user;
  cns_tres max_tres_per_account;
} cns_submit_qos;

/* PartitionResourceLimit (AccountDefs.h:163-175), the fields the submit checks read. */
typedef struct cns_submit_part_limit {
  uint32_t max_submit_jobs;
  uint32_t reserved0;
  int64_t max_wall_duration_per_job_sec;
  cns_tres max_tres_per_job;
} cns_submit_part_limit;

/* Limits, usage and counters before the batch.  Everything is copied.  Table shapes as in cns_limit_tables. */
typedef struct cns_submit_tables {
  uint32_t num_users, num_user_accts, num_accounts, num_qos, num_partitions, num_part_limits;
  cns_gres_layout gres;                     /* names the components of every cns_tres / cns_usage here (the call needs no node snapshot) */
  const cns_submit_qos* qos;                /* [num_qos]                                                          */
  const uint32_t* acct_parent;              /* [num_accounts] parent account or CNS_LIM_NONE (root)               */
  const cns_submit_part_limit* part_limits; /* [num_part_limits]                                                  */
  const uint32_t* user_part_limit;          /* [num_user_accts*num_partitions] index into part_limits or CNS_LIM_NONE; NULL = none */
  const uint32_t* acct_part_limit;          /* [num_accounts*num_partitions]; NULL = none                         */
  const cns_usage* user_qos;                /* [num_users*num_qos] read for jobs_count, resource; NULL = 0        */
  const cns_usage* user_part;               /* [num_user_accts*num_partitions] not read by the submit checks; may be NULL */
  const cns_usage* acct_qos;                /* [num_accounts*num_qos]; NULL = 0                                   */
  const cns_usage* acct_part;               /* [num_accounts*num_partitions] not read; may be NULL                */
  const cns_usage* qos_usage;               /* [num_qos] jobs_count, resource, wall_sec; NULL = 0                 */
  const uint32_t* user_qos_submit;          /* submit_jobs_count of the five tables, same shapes; NULL = 0        */
  const uint32_t* user_part_submit;
  const uint32_t* acct_qos_submit;
  const uint32_t* acct_part_submit;
  const uint32_t* qos_submit;
  const uint8_t* user_exists;               /* [num_users]    m_user_meta_map_.contains;    NULL = none exists    */
  const uint8_t* acct_exists;               /* [num_accounts] m_account_meta_map_.contains; NULL = none exists    */
  const uint8_t* qos_exists;                /* [num_qos]      m_qos_meta_map_.contains;     NULL = none exists    */
} cns_submit_tables;

/* What the job table of validity does not carry.  [J] = jobs->num_jobs, arrival order. */
typedef struct cns_submit_keys {
  const uint32_t* user;        /* < num_users                                                      */
  const uint32_t* user_acct;   /* < num_user_accts, or CNS_LIM_NONE: the account is not one of the user's (:703) */
  const uint32_t* account;     /* < num_accounts: job.account_chain.front()                        */
  const uint32_t* qos;         /* < num_qos                                                        */
  const uint32_t* count;       /* array job: number of children, else 1                            */
  const uint8_t* skip;         /* non-zero: failed validity or an earlier check of the caller; NULL = 0 */
} cns_submit_keys;

/* Results, caller-allocated. */
typedef struct cns_submit_out {
  uint8_t* code;             /* [J] cns_submit_code */
  int64_t* time_limit_out;   /* [J] */
  uint64_t* num_admitted;    /* may be NULL */
} cns_submit_out;

typedef struct cns_submit_timing {
  double h2d_ms;
  double prep_ms;             /* k_sub_prep: requests, static checks, items                           */
  double admit_ms;            /* the sort, the bracketing rounds and the final pass, or the ordered kernel */
  double d2h_ms;
  uint64_t candidates;        /* jobs that reach the entity checks (no failure in steps 1 - 9)         */
  uint64_t admitted;
  uint32_t rounds;            /* bracketing rounds of the parallel pass (0: not used)                  */
  uint32_t ordered_fallback;  /* 1: the ordered single-wave kernel decided (CNS_SUBMIT_MODE=seq, or the rounds did not converge) */
} cns_submit_timing;

int cns_set_submit_limits(cns_handle* h, const cns_submit_tables* t);

/* jobs: the table cns_validate_jobs takes; read for partition, time_limit_sec, node_cpu_raw, node_mem, task_cpu_raw, task_mem, node_num,
 * ntasks, gres_total and gres_spec.  flags & CNS_SUBMIT_CARRY: start from the counters and exists bits the previous call left;
 * without it from the tables of the last cns_set_submit_limits. */
int cns_check_submissions(cns_handle* h, const cns_job_soa* jobs, const cns_submit_keys* keys, uint32_t flags, const cns_submit_out* out);

/* The five submit-count tables and the three exists arrays after the last call (after cns_set_submit_limits: as set); shapes as in
 * cns_submit_tables; any pointer may be NULL. */
int cns_get_submit_usage(cns_handle* h, uint32_t* user_qos_submit, uint32_t* user_part_submit, uint32_t* acct_qos_submit,
                         uint32_t* acct_part_submit, uint32_t* qos_submit, uint8_t* user_exists, uint8_t* acct_exists, uint8_t* qos_exists);

int cns_get_submit_timing(const cns_handle* h, cns_submit_timing* t);

/* Where the kernels' paths change: jobs per workgroup of k_sub_prep, sorted items per workgroup of a round, and the rounds after which
 * the ordered kernel takes over. */
int cns_submit_shape(uint32_t* job_chunk, uint32_t* item_chunk, uint32_t* max_rounds);

#ifdef __cplusplus
}
#endif
#endif /* CRANE_GPU_SUBMIT_LIMITS_H_ */
