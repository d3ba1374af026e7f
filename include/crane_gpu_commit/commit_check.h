/*
 * crane_gpu_commit/commit_check.h — the commit loop's checks between NodeSelect and the admission: did anything take resources away
 * while the cycle was selecting, and are the jobs a placement preempts still alive?
 * (A directory of its own beside crane_gpu/, as crane_gpu_probe/, crane_gpu_resv/ and crane_gpu_valid/: that directory's file list is
 * the pinned ABI 4 surface, tests/test_abi.py; this header adds calls and changes no existing struct, so CNS_ABI_VERSION stays 4.)
 *
 * After NodeSelect returns (src/CraneCtld/JobScheduler.cpp:1441) the reference's ScheduleThread_ does three things per pending job, in
 * this order: the resource-reduce check (:1464-1540), the preempted-still-alive check (:1542-1555), and the license and run-limit
 * admission (:1557-1573).  cns_apply_run_limits (crane_gpu/run_limits.h) is the third; this call is the first two, for the whole queue
 * of the last cycle at once.  Its codes become cns_limit_job_soa::skip: a job with a code other than CNS_COMMIT_OK is one the commit
 * loop `continue`d before the admission.  Licenses (:1557-1563) stay with the caller.
 *
 * The call reads the last cycle's results where they are on the device (start, reason and the node of every placement record:
 * cns_device_results) and the events the caller uploads with it.  Per job the code is the FIRST failing check, in the reference's
 * order (all integers, no tolerance):
 *   1. gone[j] != 0                                  CNS_COMMIT_GONE            :1493-1500: `continue` before the reason is looked at
 *   2. the cycle's reason[j] != 0                    CNS_COMMIT_NOT_STARTED     :1507-1510
 *   3. reservation[j] == CNS_RESV_NONE (:1512): any placement record of the job names a node n with change[n] < end
 *                                                    CNS_COMMIT_RESOURCE_CHANGED :1514-1519
 *        change[n] = the least ev_time_sec over the node events that name n (:1479-1483: `it->second > end_time` replaces, so the
 *                    least time wins whatever the order of the events), +infinity when no event names n (:1516);
 *        end       = start_sec[j] + time_limit_sec[j] (job->end_time, :6772), saturating at INT64_MAX as absl::Time does;
 *        the comparison is strict (:1517): change == end keeps the job.  The loop has no `break` (:1514-1520), which changes
 *        nothing of the result.  Records that carry CNS_NODE_NONE are skipped.
 *   4. reservation[j] != CNS_RESV_NONE: looked at only when the reservation is in ar_resv (:1521); node events do not touch such a job.
 *        !ar_exists                                  CNS_COMMIT_RESV_DELETED    :1524-1525
 *        else ar_end_sec < end                       CNS_COMMIT_RESV_ENDS_EARLY :1526-1527
 *        else a placed node is not in ar_nodes       CNS_COMMIT_RESV_CHANGED    :1529-1533
 *   5. preempt_offsets given: an entry of the job's list with bit 31 clear (a running reference: std::get_if<RnJobInScheduler*>, :1544)
 *      whose running_alive[entry] != 0 (:1546)       CNS_COMMIT_WAITING_PREEMPTION :1551-1552
 *      Entries with CNS_PREEMPT_REF_PENDING set are skipped (:1545).
 *   6. otherwise                                     CNS_COMMIT_OK              reaches :1557
 * counts[c] = the number of jobs with code c.
 *
 * Input rules.  CNS_ERR_STATE before a successful cycle on this handle (cns_select, cns_select_preempt, cns_run_resident).
 * CNS_ERR_INVALID_ARG for: num_jobs different from the last cycle's; a missing array (time_limit_sec, out->code, an offsets array
 * without its list, running_alive when a list holds a running reference); offsets that decrease; a node index >= num_nodes; an ar_resv
 * >= the cycle's num_resv or named twice; a running reference >= num_running; a node twice inside one reservation list.  A node
 * twice inside one node event is allowed (the reference's fold takes it).  num_jobs == 0 with the last cycle's J == 0 is CNS_OK and
 * writes only counts.  Never a device fault; no kernel of the call waits for another workgroup.
 *
 * The call writes only device buffers of its own: a cns_download, cns_probe, cns_resvq_run, cns_validate_jobs or
 * cns_apply_run_limits before or after it behaves exactly as without it.  Every call uploads its own events, so a new cycle or a
 * cns_set_nodes invalidates nothing the caller can see.  Ownership, errors, threading: as in node_select.h.  No CPU fallback.
 *
 * NOT served: the multi-device group (cns_group_*: it merges the devices' results on the host, so there is no one device that holds
 * the cycle's results); call it on a single handle, or restate :1464-1555 over the merged placements.
 */
#ifndef CRANE_GPU_COMMIT_CHECK_H_
#define CRANE_GPU_COMMIT_CHECK_H_

#include <stdint.h>

#include "../crane_gpu/node_select.h"
#include "../crane_gpu/preempt.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CNS_CC_TIME_INFINITE_PAST INT64_MIN /* absl::InfinitePast(): CranedDown / drain events, CranedMetaContainer.cpp:111,898,941 */

typedef enum cns_commit_code {
  CNS_COMMIT_OK = 0,                 /* reaches MallocLicense / CheckAndMallocMetaResource (:1557) */
  CNS_COMMIT_GONE = 1,               /* caller's gone[j]: not in the pending map any more (:1493-1500) */
  CNS_COMMIT_NOT_STARTED = 2,        /* the cycle left a reason (:1507-1510), ENGINE_REFUSED included */
  CNS_COMMIT_RESOURCE_CHANGED = 3,   /* "Resource changed"      :1518 */
  CNS_COMMIT_RESV_DELETED = 4,       /* "Reservation deleted"   :1525 */
  CNS_COMMIT_RESV_ENDS_EARLY = 5,    /* "Resource"              :1527 */
  CNS_COMMIT_RESV_CHANGED = 6,       /* "Reservation changed"   :1531 */
  CNS_COMMIT_WAITING_PREEMPTION = 7  /* "Waiting for Preemption" :1552 */
} cns_commit_code;

/* g_meta_container->LockAndGetResReduceEvents() (:1468-1486), split by alternative: node events and affected reservations. */
typedef struct cns_commit_events {
  uint32_t num_node_events, num_affected_resv;
  const int64_t* ev_time_sec;   /* [E]   affected_nodes.first (:1477) */
  const uint64_t* ev_offsets;   /* [E+1] CSR: affected_nodes.second (:1478) ... */
  const uint32_t* ev_nodes;     /*       ... as node indices of the snapshot */
  const uint32_t* ar_resv;      /* [A] index into the cns_resv_soa of the cycle; distinct (affected_resv_set, :1472) */
  const uint8_t* ar_exists;     /* [A] GetResvMetaPtr() != nullptr NOW (:1524) */
  const int64_t* ar_end_sec;    /* [A] resv_meta->end_time NOW (:1526); not read where !ar_exists */
  const uint64_t* ar_offsets;   /* [A+1] CSR: resv_meta->craned_ids NOW (:1530); empty where !ar_exists */
  const uint32_t* ar_nodes;
} cns_commit_events;

/* The pending queue of the last cycle, in its order: [J] = that cycle's num_jobs. */
typedef struct cns_commit_jobs {
  uint64_t num_jobs;
  const int64_t* time_limit_sec;    /* as given to the cycle: end = start + limit (:6772) */
  const uint32_t* reservation;      /* as given to the cycle; NULL = none */
  const uint8_t* gone;              /* NULL = 0 */
  const uint64_t* preempt_offsets;  /* [J+1] cns_preempt_out::offsets of the cycle; NULL = no lists */
  const uint32_t* preempted;        /* cns_preempt_out::preempted */
  uint32_t num_running, reserved0;
  const uint8_t* running_alive;     /* [num_running] m_running_job_map_.contains(id) NOW (:1546) */
} cns_commit_jobs;

/* Results, caller-allocated. */
typedef struct cns_commit_out {
  uint8_t* code;     /* [J] cns_commit_code */
  uint64_t* counts;  /* [8] jobs per code; may be NULL */
} cns_commit_out;

/* After a successful cycle.  ev == NULL: no events.  kernel_ms (may be NULL): HIP-event time of the call's kernels. */
int cns_commit_check(cns_handle* h, const cns_commit_events* ev, const cns_commit_jobs* jobs, const cns_commit_out* out,
                     double* kernel_ms);
/* Where the check kernel's paths change: jobs per workgroup, and the most placement records a single lane walks (a wider job is
 * the whole wave's). */
int cns_commit_shape(uint32_t* job_chunk, uint32_t* lane_max_nodes);

#ifdef __cplusplus
}
#endif
#endif /* CRANE_GPU_COMMIT_CHECK_H_ */
