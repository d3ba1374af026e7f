/*
 * crane_gpu_running/running_attrs.h — the per-job attributes of the running set kept beside the device ledger (running.h), and the
 * two calls that read a running job's attributes from there instead of from the host: the MultiFactorPriority sorter in front of a
 * cycle (crane_gpu/priority.h) and the cycle with preemption (running_preempt.h).
 * (A header of its own beside running.h and running_preempt.h: no existing struct or call changes, CNS_ABI_VERSION stays 4.)
 *
 * Reference (paths relative to the CraneSched tree):
 *   what the sorter reads of a running job                             src/CraneCtld/JobScheduler.cpp:7692-7746
 *   allocated_res_view = the sum of allocated_res over the nodes       src/CraneCtld/CtldPublicDefs.cpp:1901-1902, JobScheduler.h:74,89
 *   what TryPreempt_ reads of a running job                            src/CraneCtld/JobScheduler.cpp:6378-6505
 *
 * THE COLUMNS.  Five values per ledger row, always in LEDGER ORDER: start_sec (i64), qos (u32), qos_priority (u32),
 * partition_priority (u32), account (u32, the dense id of crane_gpu/priority.h).  A ledger either carries all five or none.
 *
 * cns_running_seed_attrs(h, rn, job_ids, attrs): cns_running_seed (same rules, same refusals, same per-slot tables), plus the five
 * arrays [rn->num_jobs] of `attrs` copied into the columns.  attrs == NULL or a NULL array with a non-empty set:
 * CNS_ERR_INVALID_ARG.  An empty set gives an empty ledger WITH (empty) columns.
 *
 * cns_running_advance_attrs(h, in, queue_attrs, out): cns_running_advance — the same three steps, the same refusals, the same
 * results — with the columns following the rows: a retire erases a row's attributes with it, stably; an admitted row takes qos,
 * qos_priority, partition_priority and account of its queue job j from queue_attrs ([in->num_jobs], queue order) and
 * start_sec = in->now_sec (the job starts now; queue_attrs->start_sec is NOT read).  queue_attrs and its four arrays are required
 * when in->num_jobs != 0 (CNS_ERR_INVALID_ARG).  CNS_ERR_STATE when the ledger carries no columns.  As in cns_running_advance the
 * call writes copies and swaps them in on success: a refusal leaves ledger, per-slot tables and columns as they were.
 *
 * PLAIN CALLS DROP THE COLUMNS.  cns_running_seed and cns_running_advance on a ledger with columns behave exactly as ever and leave
 * a ledger without columns; everything that drops the ledger (cns_set_running, a changed num_nodes) drops them too.  The consumers
 * below then return CNS_ERR_STATE with a message that says so.
 *
 * THE DERIVED VALUES.  Per row, computed on the device once per ledger state and kept until the next seed / advance:
 *   node_num       the row's number of allocations
 *   alloc_cpu_raw  the sum of alloc_cpu_raw over the row's allocations
 *   alloc_mem      the sum of alloc_mem over the row's allocations
 * (one lane sums a row of at most lane_max_allocs allocations, a wider row is handed to its wave: cns_running_shape).  The sums are
 * taken exactly (128-bit); a row whose cpu sum is negative or leaves int64, or whose memory sum leaves uint64, is recorded and
 * refused by cns_priority_order_resident; cns_running_get_attrs reports the low 64 bits for such a row.
 *
 * cns_running_get_attrs downloads the columns and the three derived values (every pointer optional, capacity as in cns_running_get).
 *
 * cns_priority_order_resident(h, now, cfg, num_accounts, pd, limit, order_out, priority_out, num_ordered): cns_priority_order with
 * the running side taken from the ledger: running job i is ledger row i, so an account's fp64 service value is accumulated in
 * ledger order; results are bit for bit those of cns_priority_order fed the same rows.  The per-account CSR, the presence flags and
 * the input rules of the running side are device work:
 *   a row whose account >= num_accounts                                     CNS_ERR_INVALID_ARG
 *   a row whose cpu sum is negative                                         CNS_ERR_INVALID_ARG
 *   a row whose cpu sum leaves int64 or whose memory sum leaves uint64      CNS_ERR_UNSUPPORTED
 * the least offending row decides and the message names it; nothing is written to the outputs on a refusal.  The pending side is
 * uploaded and checked as in cns_priority_order.  An empty ledger means no running jobs.  CNS_ERR_STATE without a ledger or
 * without columns.  cns_priority_timing reports this call when it was the last one.
 *
 * cns_running_select_preempt_attrs: cns_running_select_preempt with rn_qos, rn_qos_priority and rn_start_sec taken from the columns
 * (device-to-device copies) and without the id check: the rows are the ledger's by construction.  With preemption enabled
 * preempt->rn_job_id, rn_qos, rn_qos_priority and rn_start_sec must be NULL (CNS_ERR_INVALID_ARG: a caller who hands them in
 * believes they are read); CNS_ERR_STATE without columns.  preempt == NULL or enabled == 0: exactly cns_running_select_preempt.
 * The admit step of cns_running_advance / cns_running_advance_attrs behind it is served as behind cns_running_select_preempt
 * (in->admit required).
 *
 * Limits are those of running.h, running_preempt.h and priority.h.  Never a device fault: every index a kernel follows is validated
 * on the host or bounded in the kernel.  No kernel of these calls waits for another workgroup.  No pass over all running jobs runs
 * on a host thread.  Single device only (not served through cns_group_*).  Ownership, errors, threading: as in node_select.h.
 * There is no CPU fallback.
 */
#ifndef CRANE_GPU_RUNNING_ATTRS_H_
#define CRANE_GPU_RUNNING_ATTRS_H_

#include <stdint.h>

#include "../crane_gpu/priority.h"
#include "running.h"
#include "running_preempt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The attributes handed in: [rn->num_jobs] rows at a seed, [in->num_jobs] queue jobs at an advance. */
typedef struct cns_running_attrs {
  const int64_t* start_sec;            /* job->start_time (not read at an advance: an admitted row starts at in->now_sec) */
  const uint32_t* qos;                 /* dense QoS id, as cns_preempt_soa::rn_qos                                       */
  const uint32_t* qos_priority;
  const uint32_t* partition_priority;
  const uint32_t* account;             /* dense account id, as cns_prio_running_soa::account                             */
} cns_running_attrs;

/* Where cns_running_get_attrs writes; every pointer may be NULL.  capacity_jobs: elements the arrays hold (CNS_ERR_INVALID_ARG when
 * the ledger is larger); *num_jobs is written first (a call with NULL arrays asks for it). */
typedef struct cns_running_attrs_out {
  uint64_t capacity_jobs;
  uint64_t* num_jobs;
  int64_t* start_sec;                  /* [jobs] the columns        */
  uint32_t* qos;
  uint32_t* qos_priority;
  uint32_t* partition_priority;
  uint32_t* account;
  uint32_t* node_num;                  /* [jobs] the derived values */
  int64_t* alloc_cpu_raw;
  uint64_t* alloc_mem;
} cns_running_attrs_out;

int cns_running_seed_attrs(cns_handle* h, const cns_running_soa* rn, const uint32_t* job_ids, const cns_running_attrs* attrs);
int cns_running_advance_attrs(cns_handle* h, const cns_running_step* in, const cns_running_attrs* queue_attrs,
                              const cns_running_step_out* out);
int cns_running_get_attrs(cns_handle* h, const cns_running_attrs_out* out);
int cns_priority_order_resident(cns_handle* h, int64_t now_sec, const cns_priority_config* cfg, uint32_t num_accounts,
                                const cns_prio_pending_soa* pd, uint64_t limit, uint32_t* order_out, double* priority_out,
                                uint64_t* num_ordered);
int cns_running_select_preempt_attrs(cns_handle* h, int64_t now_sec, const cns_job_soa* jobs, const cns_preempt_soa* preempt,
                                     cns_placement_soa* out, cns_preempt_out* pout);

#ifdef __cplusplus
}
#endif
#endif /* CRANE_GPU_RUNNING_ATTRS_H_ */
