/*
 * crane_gpu_amend/running_amend.h — change the end time of running jobs on the device-resident running set (the ledger of
 * crane_gpu_running/running.h), and seed the reservation what-ifs' per-node tables (crane_gpu_resv/resv_probe.h) from that ledger.
 * (A directory of its own: the file lists of crane_gpu/ and crane_gpu_running/ are pinned, tests/test_abi.py and
 * tests/test_running_abi.py; this header adds calls and changes no existing struct, so CNS_ABI_VERSION stays 4.)
 *
 * Reference (paths relative to the CraneSched tree):
 *   JobScheduler::ChangeJobTimeConstraint                               src/CraneCtld/JobScheduler.cpp:2211-2455
 *   ... SetEndTime of the running job                                   src/CraneCtld/JobScheduler.cpp:2411-2413
 *   ... the new end, EffectiveJobEndTimeAfterTimeConstraintChange_      src/CraneCtld/JobScheduler.cpp:116-123
 *   ... an array parent reaches every running child                     src/CraneCtld/JobScheduler.cpp:2312-2321
 *   ... a job that does not exist: ERR_NON_EXISTENT                     src/CraneCtld/JobScheduler.cpp:2302-2305
 *   JobScheduler::ResumeSuspendedJobs: the end moves out                src/CraneCtld/JobScheduler.cpp:2833-2857
 *   the running jobs' end_time folded into the next cycle's node states src/CraneCtld/JobScheduler.cpp:6681-6709
 *   CreateResv_'s walk over the running jobs' end times                 src/CraneCtld/JobScheduler.cpp:4391-4400
 * Deciding the new end (deadline, suspended duration, the reservation-end checks of :2273-2298) stays with the caller.
 *
 * cns_running_amend_ends(h, in, out): every ledger row whose job id is one of in->job_ids[i] gets in->end_sec[i].  An id that no row
 * carries changes nothing and reports out->found[i] = 0 (the reference's ERR_NON_EXISTENT; it is the caller's to report).  Row order,
 * ids, reservations and allocations do not move.  Only the end column of the ledger and, when the per-slot running tables are the
 * ledger's, their end times are written: which slot an allocation lands on, and in which order, depends on the row order and the
 * layout alone, so the tables' offsets and resources stay, and each table entry takes the end of the row that owns its allocation —
 * exactly what cns_running_seed of the amended ledger would leave.  No sort, no expansion; the only upload is the K amendments.
 *   When the per-slot tables are stale (after cns_set_nodes / cns_set_reservations, before the next cns_running_advance) only the
 *   ledger is written; the advance that must follow rebuilds from it, as ever (cns_running_amend_timing::pairs == 0 says so).
 *   The attribute columns of running_attrs.h and their derived sums stay valid: no row moves, and the sums (node_num, cpu, mem per row)
 *   are taken from a row's allocation range and its allocations' resources (running_attrs_kernels.inc: k_ra_sums reads the ledger's
 *   offsets and resources, never an end).
 *   The preempt index of running_preempt.h carries entry ends: it is cleared, the next cns_running_select_preempt builds it again
 *   (cns_debug_get_preempt_index is refused until then).
 *   The results of the last cycle stay where they are: cns_probe, cns_commit_check, cns_usage_apply and the admit step of a
 *   cns_running_advance behind the call behave exactly as without it.  cns_run_resident after the call runs on the amended ends.
 *   The tables of cns_resvq_set_state / cns_resvq_set_state_resident are buffers of their own and keep their state until set again.
 *   The call writes copies and swaps them in on success: a call that fails leaves the ledger, the tables, the columns and the preempt
 *   index as they were.  num_amend == 0: CNS_OK, nothing is written.
 *   REFUSALS: null handle or `in`: CNS_ERR_INVALID_ARG; no ledger (before cns_running_seed, after cns_set_running or a changed
 *   num_nodes): CNS_ERR_STATE; a missing array, or an id that stands twice in job_ids: CNS_ERR_INVALID_ARG; more than 2^32 - 256
 *   amendments: CNS_ERR_UNSUPPORTED.
 *
 * cns_resvq_set_state_resident(h, resv): cns_resvq_set_state with the running side taken from the ledger where it is — latest_end per
 * node over the ledger's end, offset and node arrays on the device; the reservation side from `resv` exactly as cns_resvq_set_state.
 * CNS_ERR_STATE without a ledger or before cns_set_nodes.  An empty ledger: no running allocations.  The tables do not follow later
 * amends or advances by themselves: the caller sets them again, as with cns_resvq_set_state.
 *
 * Never a device fault: every index a kernel follows is validated on the host or bounded in the kernel.  No kernel of these calls
 * waits for another workgroup.  Single device only (not served through cns_group_*).  Ownership, errors, threading: as in
 * node_select.h.  There is no CPU fallback.
 */
#ifndef CRANE_GPU_RUNNING_AMEND_H_
#define CRANE_GPU_RUNNING_AMEND_H_

#include <stdint.h>

#include "../crane_gpu/node_select.h"
#include "../crane_gpu_resv/resv_probe.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct cns_running_amend {
  uint64_t num_amend;
  const uint32_t* job_ids;   /* [K] any order, distinct                               */
  const int64_t* end_sec;    /* [K] the job's new end_time, whole seconds, any value  */
} cns_running_amend;

typedef struct cns_running_amend_out {
  uint8_t* found;            /* [K] 1: a ledger row carried job_ids[i]; required when K != 0 */
  uint64_t* num_amended;     /* may be NULL: rows written                              */
} cns_running_amend_out;

typedef struct cns_running_amend_timing {
  double h2d_ms, kernels_ms, d2h_ms;
  uint64_t rows, pairs;      /* ledger rows walked; table entries refilled (0: tables were not the ledger's) */
} cns_running_amend_timing;

int cns_running_amend_ends(cns_handle* h, const cns_running_amend* in, const cns_running_amend_out* out);
int cns_running_amend_get_timing(const cns_handle* h, cns_running_amend_timing* t);
int cns_resvq_set_state_resident(cns_handle* h, const cns_resv_soa* resv);

#ifdef __cplusplus
}
#endif
#endif /* CRANE_GPU_RUNNING_AMEND_H_ */
