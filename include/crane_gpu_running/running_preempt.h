/*
 * crane_gpu_running/running_preempt.h — a cycle with preemption on the running set that lives on the device (running.h): the index
 * cns_select_preempt derives on the host from the arrays of cns_set_running (which running job owns an entry of the per-slot tables,
 * the entries of every running job, the ends of the jobs in m_preempting_set_) is built on the device from the ledger.
 * (A header of its own beside running.h: no existing struct changes, CNS_ABI_VERSION stays 4.)
 *
 * Reference (paths relative to the CraneSched tree):
 *   m_preempting_set_: ids no longer running dropped, the others end at now + 1      src/CraneCtld/JobScheduler.cpp:6545-6559
 *   LocalScheduler::TryPreempt_                                                       src/CraneCtld/JobScheduler.cpp:6378-6505
 *   a running job's end inside TryPreempt_                                            src/CraneCtld/JobScheduler.cpp:6513-6514
 *   the commit loop holds a job that preempted back ("Waiting for Preemption")       src/CraneCtld/JobScheduler.cpp:1542-1555
 *
 * cns_running_select_preempt is cns_select_preempt (crane_gpu/preempt.h: same structs, same results, same limits) for a handle whose
 * per-slot running tables were built by cns_running_seed / cns_running_advance.
 *   RUNNING INDEX  running job index r is LEDGER ROW r: preempt->rn_job_id, rn_qos, rn_qos_priority and rn_start_sec are [ledger rows]
 *           in LEDGER ORDER (seed order, stable erase, appended in queue order; cns_running_get reports it), and a reference
 *           without bit 31 in pout->preempted is a ledger row.
 *   ID CHECK  rn_job_id is compared with the ledger's job_id column on the device; the first row that differs is
 *           CNS_ERR_INVALID_ARG with a message that names the row and both ids.  Nothing of the cycle has run at that point: the
 *           queue, the results of the last cycle and every table of the handle are as before the call.
 *   ORDER   CNS_ERR_STATE before a ledger exists, and when the per-slot tables are not the ledger's: after cns_set_running, and after
 *           cns_set_nodes / cns_set_reservations without the cns_running_advance that follows them.
 *   OFF     preempt == NULL or enabled == 0: exactly cns_select (pout may be NULL), the set passes through.
 *   THE SET ids of preempt->preempting_job_ids that no ledger row carries are dropped; the rows of the others end at now + 1 FOR THIS
 *           CALL ONLY: the call patches a copy of the per-slot end times and binds it for its cycle; the resident end times are never
 *           written.  An id may stand twice.
 *   NO LIST enabled, but no pending job's QoS has a preempt list: the plain cycle on the pipelined kernels with the patched ends.
 *   cns_select_preempt itself keeps refusing device-built tables.  The admit step of cns_running_advance IS served after a successful
 *   call (running.h).  cns_probe after such a cycle stays refused, as after cns_select_preempt.
 * Never a device fault: every index a kernel follows is validated on the host or bounded in the kernel.  No kernel of the call waits
 * for another workgroup.  Single device only (not served through cns_group_*).  No pass over all running jobs or all per-slot entries
 * runs on a host thread.  Ownership, errors, threading: as in node_select.h.  There is no CPU fallback.
 *
 * THE INDEX.  Entry d of the per-slot tables is position d of the rebuild's (slot, ledger allocation) pairs sorted by slot:
 *   ent_slot[d]  the slot;  ent_job[d]  the ledger row that owns the allocation;
 *   rj_off / rj_ent  the entries of row r in ascending d (a row without an entry — an allocation on an unschedulable node, an unknown
 *           reservation, a reservation that does not list the node — has an empty range);
 * built by the first call after a cns_running_seed / cns_running_advance and kept until the next one.  Per call: rj_preempting[r],
 * rj_end[r] = max(end of the row after the patch, now + 1) for a row with an entry, else 0, and the patched per-entry ends.
 * cns_debug_get_preempt_index downloads all of it as the last cns_running_select_preempt with preemption enabled left it (every pointer
 * optional; CNS_ERR_STATE before such a call, and after a cns_running_seed / cns_running_advance / change of the layout behind it).
 */
#ifndef CRANE_GPU_RUNNING_PREEMPT_H_
#define CRANE_GPU_RUNNING_PREEMPT_H_

#include <stdint.h>

#include "../crane_gpu/preempt.h"
#include "running.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Where cns_debug_get_preempt_index writes; every pointer may be NULL.  capacity_*: elements the arrays hold (CNS_ERR_INVALID_ARG when
 * the index is larger); *num_entries / *num_rows are written first (a call with NULL arrays asks for them). */
typedef struct cns_preempt_index_out {
  uint64_t capacity_entries, capacity_rows;
  uint64_t *num_entries, *num_rows;
  uint32_t* ent_job;             /* [entries]  */
  uint32_t* ent_slot;            /* [entries]  */
  int64_t* ent_end;              /* [entries] the per-slot end times the cycle ran on */
  uint32_t* rj_off;              /* [rows + 1] */
  uint32_t* rj_ent;              /* [entries]  */
  int64_t* rj_end;               /* [rows]     */
  uint8_t* rj_preempting;        /* [rows]     */
} cns_preempt_index_out;

/* What the last cns_select_preempt / cns_running_select_preempt with preemption enabled spent in front of its cycle. */
typedef struct cns_running_preempt_timing {
  double setup_ms;       /* host clock, from the entry of the call to the launch of its cycle (cns_upload_jobs included); either call */
  double index_ms;       /* device: the entry index and the job -> entries CSR (0 when the call reused them)                         */
  double mark_ms;        /* device: the uploads of the call, the id check, the marks, rj_end and the end patch                       */
  uint64_t entries;      /* entries of the per-slot tables                                                                           */
  uint64_t rows;         /* ledger rows                                                                                              */
  uint32_t index_built;  /* 1: this call built the index                                                                             */
  uint32_t reserved0;
} cns_running_preempt_timing;

int cns_running_select_preempt(cns_handle* h, int64_t now_sec, const cns_job_soa* jobs, const cns_preempt_soa* preempt,
                               cns_placement_soa* out, cns_preempt_out* pout);
int cns_debug_get_preempt_index(cns_handle* h, const cns_preempt_index_out* out);
int cns_running_preempt_get_timing(const cns_handle* h, cns_running_preempt_timing* t);

#ifdef __cplusplus
}
#endif
#endif /* CRANE_GPU_RUNNING_PREEMPT_H_ */
