/*
 * crane_gpu_usage/usage.h — release, or charge, a batch of jobs on the account / user / QoS usage tables, on the device.
 * (A directory of its own beside crane_gpu/, as crane_gpu_probe/, crane_gpu_resv/, crane_gpu_valid/, crane_gpu_commit/, crane_gpu_submit/
 * and crane_gpu_gate/: crane_gpu/'s file list is the pinned ABI 4 surface, tests/test_abi.py; this header adds calls and changes no
 * existing struct, so CNS_ABI_VERSION stays 4.)
 *
 * Reference (paths relative to the CraneSched tree):
 *   AccountMetaContainer::DoFreeResource_ with its safe_sub          src/CraneCtld/Accounting/AccountMetaContainer.cpp:1126-1208
 *   DoMallocResource_                                               :1067-1124
 *   MetaResource::operator<=, +=, -=, SetToZero                     :33-60
 *   ResourceView / GresCount operator<=                             src/Utilities/PublicHeader/PublicHeader.cpp:57-69, :648-659
 *   the callers: FreeMetaSubmitResource :226, FreeMetaResource(JobInCtld) :243, FreeMetaRunningResource :256,
 *                FreeMetaResource(PdJobInScheduler) :271, MallocMetaSubmitResource :139, MallocMetaResourceToRecoveredRunningJob :155
 *
 * What it computes.  One MetaResource = a cns_usage (resource, jobs_count, wall_time) + its submit_jobs_count: 17 integer components
 * (cpu, mem, wall, jobs, submit, 4 GRES name totals, 8 GRES class counts).  The J rows of a call are J calls of DoFreeResource_
 * (CNS_USAGE_RELEASE) or DoMallocResource_ (CNS_USAGE_CHARGE) IN THE ORDER GIVEN, each with the row's delta.  A row touches
 *     (user, qos); (user_acct, partition) unless user_acct == CNS_LIM_NONE; (a, qos) and (a, partition) for every account a from
 *     `account` to the root over acct_parent; the QoS's global record
 * which is at most 2 + 2 * CNS_LIM_MAX_CHAIN + 1 = 15 records, none of them twice.
 *
 * RELEASE, per record, with the record's rows in call order and P_k the component-wise inclusive prefix sum of their deltas
 * (safe_sub, :1138-1160: delta <= val in EVERY component -> val -= delta; otherwise the whole record := 0; a nested record that is zero
 * afterwards is erased):
 *   the record ends as val - T if the total T fits val in every component, as zero otherwise; a nested record that ends at zero no
 *   longer exists (its exists byte is 0 and its value reads as zero).  qos_usage has no exists byte and stays.
 *   row k is clean while P_k <= val.  The first row where that fails "frees more than allocated" (:1152): its over_free bit.  Every row
 *   behind it, and every row behind a k with P_k == val on a nested record (erased, :1159), finds the key gone (:1143): its not_found
 *   bit.  On the global QoS record, which is never erased (:1190-1202), every later row over-frees again.
 *   A nested record that does not exist before the call: every row's not_found bit, nothing changes.
 *   An entity (user, chain account, QoS) that does not exist (if_contains, :1162, :1180, :1190): nothing under it is touched and no bit
 *   is set for it.  Entity bits never change.  user_acct == CNS_LIM_NONE under an existing user sets bit 1 of not_found (:1172); it
 *   also stands for "the user's record has no partition map for this account": the dense model cannot tell the two apart and the
 *   table values agree either way.
 *   A prefix sum beyond 64 bits does not fit (every value is at most UINT64_MAX, so this is exact).
 * CHARGE: every touched record += delta (:1078-1084), its nested exists byte := 1, the user's, every chain account's and the QoS's
 *   entity bit := 1 (try_emplace_l).  Both masks come back 0.  A jobs_count or submit count that would pass UINT32_MAX, a cpu or wall sum
 *   beyond INT64_MAX or another component beyond UINT64_MAX: CNS_ERR_UNSUPPORTED and the tables stay as they were (the reference adds
 *   the counts in 32 bits; refused, not wrapped, as cns_check_submissions does).  user_acct == CNS_LIM_NONE in a CHARGE row is
 *   CNS_ERR_INVALID_ARG: the reference creates the partition map of account_chain.front(), which the dense model has no slot for.
 *
 * Bits of not_found[j] / over_free[j]: 0 user_qos, 1 user_part, 2 + 2i / 3 + 2i acct_qos / acct_part of the i-th chain account
 * (0 = the job's account), 14 the QoS.
 *
 * Input rules.  CNS_ERR_STATE: cns_usage_apply / cns_usage_get_tables before cns_usage_set_tables; CNS_USAGE_CARRY before a first
 * cns_usage_apply that succeeded.  CNS_ERR_INVALID_ARG: a missing required array (the five key arrays, out->not_found, out->over_free),
 * an unknown op; in a row that is not skipped an index out of range (user_acct: in range or CNS_LIM_NONE), a negative cpu_raw or
 * wall_sec, a delta that is all zero (the reference returns before DoFreeResource_ for it, :228; the caller skips it); in the tables
 * an acct_parent out of range or a chain that does not end, a negative cpu_raw or wall_sec, a bad gres layout.  CNS_ERR_UNSUPPORTED:
 * a chain of more than CNS_LIM_MAX_CHAIN accounts, more than CNS_USAGE_MAX_JOBS rows in one call, more than 2^32 - 16 records.
 * num_jobs == 0 is CNS_OK and writes nothing.  Never a device fault; no kernel of the call waits for another workgroup.  Single device
 * only (not served through cns_group_*).  The call reads and writes device buffers of its own: a cycle, cns_apply_run_limits or
 * cns_check_submissions before or after it behaves exactly as without it; a later change can seed those calls' resident tables from
 * these device to device, in either direction.  Ownership, errors, threading: as in node_select.h.  There is no CPU fallback.
 *
 * With the caller: UserAddJob / UserReduceJob (:169, :1207), DeleteUserMeta / DeleteAccountMeta / DeleteQosMeta.
 */
#ifndef CRANE_GPU_USAGE_H_
#define CRANE_GPU_USAGE_H_

#include <stdint.h>

#include "../crane_gpu/run_limits.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CNS_USAGE_RELEASE 0u        /* op: DoFreeResource_ per row   */
#define CNS_USAGE_CHARGE 1u         /* op: DoMallocResource_ per row */
#define CNS_USAGE_CARRY 1u          /* flags: start from what the previous cns_usage_apply left */
#define CNS_USAGE_MAX_JOBS 16777216u /* rows of one call */
#define CNS_USAGE_BIT_USER_QOS 0
#define CNS_USAGE_BIT_USER_PART 1
#define CNS_USAGE_BIT_ACCT_QOS(i) (2 + 2 * (i))
#define CNS_USAGE_BIT_ACCT_PART(i) (3 + 2 * (i))
#define CNS_USAGE_BIT_QOS 14

/* The tables before the first call.  Everything is copied.  Shapes as in cns_limit_tables / cns_submit_tables. */
typedef struct cns_usage_tables {
  uint32_t num_users, num_user_accts, num_accounts, num_qos, num_partitions, reserved0;
  cns_gres_layout gres;                /* names the components of every cns_usage here (the call needs no node snapshot) */
  const uint32_t* acct_parent;         /* [num_accounts] parent account or CNS_LIM_NONE (root)            */
  const cns_usage* user_qos;           /* [num_users*num_qos]; NULL = 0                                   */
  const cns_usage* user_part;          /* [num_user_accts*num_partitions]                                 */
  const cns_usage* acct_qos;           /* [num_accounts*num_qos]                                          */
  const cns_usage* acct_part;          /* [num_accounts*num_partitions]                                   */
  const cns_usage* qos_usage;          /* [num_qos]                                                       */
  const uint32_t* user_qos_submit;     /* submit_jobs_count of the five tables, same shapes; NULL = 0     */
  const uint32_t* user_part_submit;
  const uint32_t* acct_qos_submit;
  const uint32_t* acct_part_submit;
  const uint32_t* qos_submit;
  const uint8_t* user_qos_exists;      /* "the map has an entry", same shapes as the four nested tables.  NULL = every entry exists if */
  const uint8_t* user_part_exists;     /* the table or its submit counts are given, none otherwise.  A record with exists == 0 is   */
  const uint8_t* acct_qos_exists;      /* read as zero, whatever its value.                                                           */
  const uint8_t* acct_part_exists;
  const uint8_t* user_exists;          /* [num_users]    m_user_meta_map_.contains;    NULL = none exists */
  const uint8_t* acct_exists;          /* [num_accounts] m_account_meta_map_.contains; NULL = none exists */
  const uint8_t* qos_exists;           /* [num_qos]      m_qos_meta_map_.contains;     NULL = none exists */
} cns_usage_tables;

/* One row per Free... / Malloc... call of the reference, in call order.  [J] = num_jobs.
 *   FreeMetaResource(JobInCtld) :243          {alloc, jobs 1, submit child ? 0 : 1, time_limit}
 *   FreeMetaRunningResource :256              {alloc, 1, 0, time_limit}
 *   FreeMetaResource(PdJobInScheduler) :271   {alloc, 1, 0, time_limit}
 *   FreeMetaSubmitResource :226               {0, 0, count, 0}
 *   MallocMetaSubmitResource :139             {0, 0, count, 0}
 *   MallocMetaResourceToRecoveredRunningJob :155   {alloc, 1, child ? 0 : 1, time_limit} */
typedef struct cns_usage_jobs {
  uint64_t num_jobs;
  const uint32_t* user;          /* < num_users                                   */
  const uint32_t* user_acct;     /* < num_user_accts, or CNS_LIM_NONE             */
  const uint32_t* account;       /* < num_accounts: account_chain.front()         */
  const uint32_t* qos;           /* < num_qos                                     */
  const uint32_t* partition;     /* < num_partitions                              */
  const int64_t* cpu_raw;        /* >= 0; NULL = 0 (as every delta array below)   */
  const uint64_t* mem;
  const int64_t* wall_sec;       /* >= 0                                          */
  const uint32_t* jobs_count;
  const uint32_t* submit_count;
  const uint64_t* name_total;    /* [J*CNS_MAX_GRES_NAMES]   GresCount.total      */
  const uint64_t* class_count;   /* [J*CNS_MAX_GRES_CLASSES] GresCount.specified  */
  const uint8_t* skip;           /* non-zero: the row is not applied; NULL = 0    */
} cns_usage_jobs;

/* Results, caller-allocated. */
typedef struct cns_usage_out {
  uint16_t* not_found;     /* [J] the CRANE_ERRORs of :1143 and :1172 */
  uint16_t* over_free;     /* [J] those of :1152 and :1196            */
  uint64_t* num_clean;     /* rows with both masks zero; may be NULL  */
} cns_usage_out;

/* Where cns_usage_get_tables writes; every pointer may be NULL.  Shapes as in cns_usage_tables. */
typedef struct cns_usage_tables_out {
  cns_usage *user_qos, *user_part, *acct_qos, *acct_part, *qos_usage;
  uint32_t *user_qos_submit, *user_part_submit, *acct_qos_submit, *acct_part_submit, *qos_submit;
  uint8_t *user_qos_exists, *user_part_exists, *acct_qos_exists, *acct_part_exists;
  uint8_t *user_exists, *acct_exists, *qos_exists;
} cns_usage_tables_out;

typedef struct cns_usage_timing {
  double h2d_ms;
  double kernels_ms;     /* items, the sort, the segmented scan and the per-record apply */
  double d2h_ms;
  uint64_t items;        /* (record, row) pairs of the call */
  uint64_t records;      /* records touched                 */
} cns_usage_timing;

int cns_usage_set_tables(cns_handle* h, const cns_usage_tables* t);

/* op: CNS_USAGE_RELEASE or CNS_USAGE_CHARGE.  flags & CNS_USAGE_CARRY: start from what the previous cns_usage_apply left; without it
 * from the tables of the last cns_usage_set_tables. */
int cns_usage_apply(cns_handle* h, uint32_t op, const cns_usage_jobs* jobs, uint32_t flags, const cns_usage_out* out);

/* The tables after the last cns_usage_apply that succeeded (after cns_usage_set_tables: as set, records that do not exist zeroed). */
int cns_usage_get_tables(cns_handle* h, const cns_usage_tables_out* out);

int cns_usage_get_timing(const cns_handle* h, cns_usage_timing* t);

/* Where the kernels' paths change: rows per workgroup of the item kernel, sorted items per workgroup of the scan, and the lanes of the
 * one workgroup that carries the scan across workgroups (each takes ceil(workgroups / carry_lanes) of them). */
int cns_usage_shape(uint32_t* job_chunk, uint32_t* item_chunk, uint32_t* carry_lanes);

#ifdef __cplusplus
}
#endif
#endif /* CRANE_GPU_USAGE_H_ */
