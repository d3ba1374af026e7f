/*
 * crane_gpu_running/running.h — keep the running set on the device between two cycles: retire the jobs that ended, admit the jobs the
 * commit loop started, rebuild the per-slot running tables, all without the caller handing the whole cns_running_soa in again.
 * (A directory of its own beside crane_gpu/, as crane_gpu_probe/, crane_gpu_resv/, crane_gpu_valid/, crane_gpu_commit/,
 * crane_gpu_submit/, crane_gpu_gate/ and crane_gpu_usage/: crane_gpu/'s file list is the pinned ABI 4 surface, tests/test_abi.py; this
 * header adds calls and changes no existing struct, so CNS_ABI_VERSION stays 4.)
 *
 * Reference (paths relative to the CraneSched tree):
 *   the running jobs folded into the node states of a cycle            src/CraneCtld/JobScheduler.cpp:6681-6709
 *   CranedMetaContainer::FreeResourceFromNode                          src/CraneCtld/CranedMetaContainer.cpp:226-277 (unknown job: :248-253)
 *   ... driven when a job ends                                         src/CraneCtld/JobScheduler.cpp:5318-5425
 *   CranedMetaContainer::MallocResourceFromNode                        src/CraneCtld/CranedMetaContainer.cpp:178-224
 *   ... driven by the commit loop for every job it starts              src/CraneCtld/JobScheduler.cpp:1575-1628
 *
 * THE LEDGER.  A job-major table on the device, in LEDGER ORDER: per job its job_id, end_sec and reservation, and a CSR of its
 * allocations (node, cpu_raw, mem, four core words, gres).  It holds the caller's node indices, so it does not depend on how the engine
 * lays the nodes out in slots; cns_set_nodes / cns_set_reservations with an unchanged num_nodes keep it.
 * Canonicalisation: the reference iterates a hash map of running jobs (order unspecified, and the initial fp64 node cost depends on
 * it: JobScheduler.h:508-510); ledger order stands in for that order.  cns_running_seed keeps the input order, a retire is a STABLE
 * erase, admitted jobs are appended in queue order.  The per-slot running tables are, per slot, in ledger order: exactly what
 * cns_set_running would derive from the ledger handed in as a cns_running_soa.
 *
 * cns_running_seed(h, rn, job_ids): copies the set into the ledger, derives the per-slot tables from it on the device and leaves them
 * exactly as cns_set_running(h, rn) would.  The rules of cns_set_running apply (a missing array, num_allocs mismatch, an allocation on
 * a node >= num_nodes: CNS_ERR_INVALID_ARG), plus: alloc_offsets start at 0 and never decrease, job_ids is given and its values are
 * distinct (CNS_ERR_INVALID_ARG); at most 2^32 - 512 jobs and 2^32 - 256 allocations (CNS_ERR_UNSUPPORTED).  rn == NULL or no jobs:
 * an empty ledger.
 *
 * cns_running_advance(h, in, out): one call per cycle boundary, three steps in this order.
 *   RETIRE  every ledger row that carries one of retire_ids[num_retire] (any order; a value twice: CNS_ERR_INVALID_ARG) is erased,
 *           stably.  out->found[i] = 0 where no row carried retire_ids[i] — the reference's "free resource from an unknown job"
 *           (CranedMetaContainer.cpp:248-253), which changes nothing either.  out->num_retired: rows erased.
 *   ADMIT   (only when in->num_jobs != 0) over the results of the last cns_select / cns_run_resident of this handle, where they are on
 *           the device: num_jobs must be that cycle's queue length (CNS_ERR_INVALID_ARG), now_sec its `now` (CNS_ERR_INVALID_ARG);
 *           without such a cycle, or after cns_select_preempt: CNS_ERR_STATE.  Job j of the queue is appended iff admit[j] != 0
 *           (NULL: every job), its reason is CNS_REASON_NONE and its start_sec == now_sec (JobScheduler.cpp:1575-1628 starts exactly
 *           these), in queue order, with job_id[j], end = start + time_limit (saturating), reservation[j] (NULL: none; it must be the
 *           array the cycle's cns_job_soa carried — the caller's contract, as in cns_commit_check), and one allocation per placement
 *           record whose node_idx != CNS_NODE_NONE, in record order.  out->num_admitted: rows appended.
 *           The ids of the admitted rows must be distinct and absent from the ledger: the caller's contract, NOT checked.
 *           After a successful cns_running_select_preempt (running_preempt.h) with preemption enabled the admit step IS served, and
 *           in->admit is required (NULL: CNS_ERR_INVALID_ARG): a job that preempted a running job has reason none and start == now,
 *           and the reference's commit loop holds it back ("Waiting for Preemption", JobScheduler.cpp:1542-1555, cns_commit_check's
 *           code) — only the caller's mask says whether it started.  A pending job preempted inside the cycle carries
 *           CNS_REASON_PREEMPTED and is never admitted.
 *   REBUILD the per-slot running tables from the new ledger against the handle's CURRENT layout: an allocation outside a reservation
 *           counts on every slot of its node (none for an unschedulable node, JobScheduler.cpp:6685-6686), one inside a reservation on
 *           that reservation's virtual node (none for an unknown reservation or one that does not list the node, :6693-6700).
 *   A call with nothing to retire and nothing to admit is what follows cns_set_nodes / cns_set_reservations (they empty the per-slot
 *   tables, as ever).  A changed num_nodes drops the ledger: the next cns_running_advance returns CNS_ERR_STATE.
 *   REFUSAL: a slot above the time map's capacity — more than 1006 allocations on a slot without reservations, or
 *   allocations + 2 * reservations + 2 > 504 with them (the check of cns_set_running) — is CNS_ERR_UNSUPPORTED and leaves the ledger AND
 *   the per-slot tables as they were before the call: the call writes copies and swaps them in on success.
 *   Also CNS_ERR_UNSUPPORTED: more than 2^32 - 512 rows / 2^32 - 256 allocations after the call, or allocations x the widest node's
 *   slots beyond 2^32 - 256.
 *
 * cns_running_get downloads the ledger (every pointer optional).  A later cns_set_running replaces the per-slot tables as ever and
 * drops the ledger.  cns_select_preempt after the tables were built here returns CNS_ERR_STATE (call cns_set_running first): its
 * setup reads the host copy of the running set, which this path does not fill; cns_running_select_preempt (running_preempt.h) is that
 * cycle on the ledger.  Never a device fault: every index a kernel follows is
 * validated on the host or bounded in the kernel.  No kernel of these calls waits for another workgroup.  Single device only (not
 * served through cns_group_*).  cns_probe, cns_commit_check, cns_usage_apply before or after behave exactly as without these calls.
 * Ownership, errors, threading: as in node_select.h.  There is no CPU fallback.
 */
#ifndef CRANE_GPU_RUNNING_H_
#define CRANE_GPU_RUNNING_H_

#include <stdint.h>

#include "../crane_gpu/node_select.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One cycle boundary.  [K] = num_retire, [J] = num_jobs (0: no admit step). */
typedef struct cns_running_step {
  uint64_t num_retire;
  const uint32_t* retire_ids;    /* [K] job ids that ended, any order, distinct                         */
  uint64_t num_jobs;             /* the last cycle's queue length, or 0                                 */
  int64_t now_sec;               /* the last cycle's now                                                */
  const uint32_t* job_id;        /* [J] id a queue job gets in the ledger                               */
  const uint8_t* admit;          /* [J] non-zero: the commit loop started the job; NULL = every job     */
  const uint32_t* reservation;   /* [J] as in the cycle's cns_job_soa; NULL = none                      */
} cns_running_step;

typedef struct cns_running_step_out {
  uint8_t* found;                /* [K] 1: a row carried retire_ids[i]; required when num_retire != 0   */
  uint64_t* num_retired;         /* may be NULL */
  uint64_t* num_admitted;        /* may be NULL */
} cns_running_step_out;

/* Where cns_running_get writes; every pointer may be NULL.  capacity_*: elements the arrays hold (CNS_ERR_INVALID_ARG when the
 * ledger is larger); *num_jobs / *num_allocs: the ledger's sizes, written first (a call with NULL arrays asks for them). */
typedef struct cns_running_ledger {
  uint64_t capacity_jobs, capacity_allocs;
  uint64_t *num_jobs, *num_allocs;
  uint32_t* job_id;              /* [jobs]     */
  int64_t* end_sec;              /* [jobs]     */
  uint32_t* reservation;         /* [jobs]     */
  uint32_t* alloc_offsets;       /* [jobs + 1] */
  uint32_t* alloc_node;          /* [allocs]   */
  int64_t* alloc_cpu_raw;
  uint64_t* alloc_mem;
  uint64_t* alloc_core_lo;
  uint64_t* alloc_core_hi;
  uint64_t* alloc_core_w2;
  uint64_t* alloc_core_w3;
  uint64_t* alloc_gres;
} cns_running_ledger;

typedef struct cns_running_timing {
  double h2d_ms;
  double kernels_ms;     /* keep / admit, the scans, the compaction, the expansion, the sort, the fill */
  double d2h_ms;
  uint64_t jobs;         /* rows of the ledger after the call          */
  uint64_t allocs;       /* its allocations                            */
  uint64_t pairs;        /* (slot, allocation) pairs of the rebuild    */
} cns_running_timing;

int cns_running_seed(cns_handle* h, const cns_running_soa* rn, const uint32_t* job_ids);
int cns_running_advance(cns_handle* h, const cns_running_step* in, const cns_running_step_out* out);
int cns_running_get(cns_handle* h, const cns_running_ledger* out);
int cns_running_get_timing(const cns_handle* h, cns_running_timing* t);

/* Where the kernels' paths change: rows per workgroup of the keep / compact kernels, allocations one lane copies alone (a wider row is
 * handed to its wave), elements per workgroup of a sort pass, per-wave counts one step of the ordered scan takes. */
int cns_running_shape(uint32_t* job_chunk, uint32_t* lane_max_allocs, uint32_t* sort_tile, uint32_t* scan_span);

#ifdef __cplusplus
}
#endif
#endif /* CRANE_GPU_RUNNING_H_ */
