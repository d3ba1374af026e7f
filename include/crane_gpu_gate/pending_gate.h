/*
 * crane_gpu_gate/pending_gate.h — the front of a scheduling cycle: which jobs of the pending map reach NodeSelect at all.
 * (A directory of its own beside crane_gpu/, as crane_gpu_probe/, crane_gpu_resv/, crane_gpu_valid/, crane_gpu_commit/ and
 * crane_gpu_submit/: that directory's file list is the pinned ABI 4 surface, tests/test_abi.py; this header adds calls and changes no
 * existing struct, so CNS_ABI_VERSION stays 4.)
 *
 * Before NodeSelect (src/CraneCtld/JobScheduler.cpp:1441) the reference's ScheduleThread_ does two things under
 * m_pending_job_map_mtx_, serially over the whole pending map:
 *   the dependency-event drain   :1353-1372   JobInCtld::UpdateDependency -> DependenciesInJob::update (CtldPublicDefs.cpp:145-160)
 *   Phase 1                      :1374-1413   Held, BeginTime, Dependency / DependencyNeverSatisfied (DependenciesInJob::is_met / is_failed,
 *                                             CtldPublicDefs.h:460-466), the array parent's gate
 *                                             (ArrayManager::PrepareParentForMaterialization, Array.cpp:683-699 ->
 *                                             ArrayMeta::SpawnBlockReason, Array.cpp:236-259)
 * cns_gate_pending is both, for every job of the pending map at once.  Its `pending` list is the pending_jobs vector of :1375-1413:
 * the rows the caller gathers its cns_prio_pending_soa / cns_job_soa from.
 *
 * Time domain.  Whole seconds in int64; INT64_MAX is absl::InfiniteFuture(), INT64_MIN is absl::InfinitePast().  `now` is whole seconds
 * in the reference (:1351).  Pass every other time rounded UP to whole seconds: with an integer now, t <= now <=> ceil(t) <= now and
 * t > now <=> ceil(t) > now, and ceil commutes with min, max and the addition of whole seconds, so no comparison of the reference
 * changes.  The sum event_time + absl::Seconds(delay) (CtldPublicDefs.cpp:153): an infinite event_time stays what it is; otherwise a
 * delay >= 2^63 gives INT64_MAX; otherwise the add saturates at INT64_MAX (abseil's documented saturating arithmetic; this rule is the
 * contract).
 *
 * Semantics, all integer and exact.
 *   1. Events, in queue order (:1361):
 *        the dependent id is not in job_id                       ignored                              :1362-1371
 *        the dependee is not in the dependent's list             ignored                              CtldPublicDefs.cpp:147-150
 *        else t = event_sec + delay of that entry                                                     CtldPublicDefs.cpp:153
 *             ready = is_or ? min(ready, t) : max(ready, t)                                           CtldPublicDefs.cpp:154-158
 *             the entry is erased                                                                     CtldPublicDefs.cpp:159
 *      so of several events that name the same (dependent, dependee) pair only the FIRST in queue order applies: the later ones find
 *      nothing.  remaining[j] = the live entries of job j minus the erased ones.
 *   2. Gate: per job the code is the FIRST failing check, in the reference's order:
 *        held[j] != 0                                            CNS_GATE_HELD                        :1380
 *        begin_sec[j] > now                                      CNS_GATE_BEGIN_TIME                  :1384
 *        !((is_or || remaining == 0) && ready <= now)            (is_met, CtldPublicDefs.h:460-462)   :1388
 *           ready == INT64_MAX && (!is_or || remaining == 0)     CNS_GATE_DEPENDENCY_NEVER            :1389-1390 (is_failed, CtldPublicDefs.h:464-466)
 *           else                                                 CNS_GATE_DEPENDENCY                  :1392
 *        array_parent[j] != 0 (:1397), in SpawnBlockReason's order:
 *           no meta (Array.cpp:686-689) or no parent pointer (:237-239)    CNS_GATE_ARRAY_NO_META     reason ""
 *           materialization complete                             CNS_GATE_ARRAY_COMPLETE              Array.cpp:240-241
 *           cancel requested                                     CNS_GATE_ARRAY_CANCELLED             Array.cpp:243-244
 *           ap_deadline_sec[j] <= now                            CNS_GATE_ARRAY_DEADLINE              Array.cpp:246-247
 *           no next task id                                      CNS_GATE_ARRAY_NO_NEXT               Array.cpp:249-250, reason ""
 *           ap_running[j] >= ap_run_limit[j]                     CNS_GATE_ARRAY_TASK_LIMIT            Array.cpp:253-256
 *           else                                                 CNS_GATE_OK_ARRAY_PARENT             :1404-1408 (materializes_array_child)
 *        otherwise                                               CNS_GATE_OK                          :1411
 *
 * Input rules.  CNS_ERR_INVALID_ARG for: a missing array (job_id, out->code / pending / num_pending; dep_is_or without dep_ready_sec or
 * the other way round; dependency entries without dep_is_or, dep_job or dep_delay_sec; array_parent without one of the ap_ arrays; events
 * without one of their three arrays); job_id not strictly ascending; dep_offsets that do not start at 0 or that decrease; a dependency
 * list that is not strictly ascending by dep_job; an ap_flags value outside the defined bits.  CNS_ERR_UNSUPPORTED above 2^32 - 512 jobs,
 * 2^32 - 256 dependency entries or 2^32 - 256 events.  num_jobs == 0 is CNS_OK: counts (all 0), ev_stats (every event ignored: no such
 * pending job) and *num_pending (0) are written, nothing else.  Never a device fault: every index the kernels follow is validated on the
 * host or bounded in the kernel.  No kernel of the call waits for another workgroup.  A failed call leaves nothing in flight.
 *
 * The call needs a handle only: no snapshot, no cycle.  It writes only device buffers of its own, so every other call on the handle
 * behaves exactly as without it.  Ownership, errors, threading: as in node_select.h.  No CPU fallback.
 *
 * NOT served here: Held() itself (the caller evaluates it), the array manager's bookkeeping behind the ap_ fields, the construction of
 * PdJobInScheduler, TriggerDependencyEvents.  The multi-device group has no call of its own: the gate reads no device state, call it on
 * any one handle.
 */
#ifndef CRANE_GPU_PENDING_GATE_H_
#define CRANE_GPU_PENDING_GATE_H_

#include <stdint.h>

#include "../crane_gpu/node_select.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CNS_GATE_TIME_INFINITE_FUTURE INT64_MAX /* absl::InfiniteFuture() */
#define CNS_GATE_TIME_INFINITE_PAST INT64_MIN   /* absl::InfinitePast(): DependenciesInJob::ready_time's initial value, CtldPublicDefs.h:458 */

typedef enum cns_gate_code {
  CNS_GATE_OK = 0,                /* pending_jobs.emplace_back                   :1411 */
  CNS_GATE_OK_ARRAY_PARENT = 1,   /* ... with materializes_array_child = true    :1404-1408 */
  CNS_GATE_HELD = 2,              /* "Held"                                      :1381 */
  CNS_GATE_BEGIN_TIME = 3,        /* "BeginTime"                                 :1385 */
  CNS_GATE_DEPENDENCY = 4,        /* "Dependency"                                :1392 */
  CNS_GATE_DEPENDENCY_NEVER = 5,  /* "DependencyNeverSatisfied"                  :1390 */
  CNS_GATE_ARRAY_NO_META = 6,     /* ""                                          Array.cpp:688, :238 */
  CNS_GATE_ARRAY_COMPLETE = 7,    /* "ArrayMaterializationComplete"              Array.cpp:241 */
  CNS_GATE_ARRAY_CANCELLED = 8,   /* "Cancelled"                                 Array.cpp:244 */
  CNS_GATE_ARRAY_DEADLINE = 9,    /* "Deadline"                                  Array.cpp:247 */
  CNS_GATE_ARRAY_NO_NEXT = 10,    /* ""                                          Array.cpp:250 */
  CNS_GATE_ARRAY_TASK_LIMIT = 11  /* "ArrayTaskLimit"                            Array.cpp:256 */
} cns_gate_code;

/* cns_gate_jobs::ap_flags */
#define CNS_GATE_AP_HAS_META 1u    /* FindMeta_(parent.JobId()) != nullptr        Array.cpp:686 */
#define CNS_GATE_AP_HAS_PARENT 2u  /* parent_job_ != nullptr                      Array.cpp:237 */
#define CNS_GATE_AP_COMPLETE 4u    /* ArrayMaterializationComplete()              Array.cpp:240 */
#define CNS_GATE_AP_CANCEL 8u      /* CancelRequested()                           Array.cpp:243 */
#define CNS_GATE_AP_HAS_NEXT 16u   /* NextMaterializableTaskId().has_value()      Array.cpp:249 */
#define CNS_GATE_AP_ALL 31u

/* m_pending_job_map_ in its btree order (:1377): [J] rows in ascending job_id. */
typedef struct cns_gate_jobs {
  uint64_t num_jobs;
  const uint32_t* job_id;          /* [J] strictly ascending */
  const uint8_t* held;             /* [J] job->Held() (:1380); NULL = 0 */
  const int64_t* begin_sec;        /* [J] job->begin_time (:1384); NULL = none */
  const uint8_t* dep_is_or;        /* [J] DependenciesInJob::is_or ... */
  const int64_t* dep_ready_sec;    /* [J] ... and ready_time, as they stand before this cycle's events; both NULL = no job has dependencies */
  const uint64_t* dep_offsets;     /* [J+1] CSR: the live entries of DependenciesInJob::deps; NULL = no entries */
  const uint32_t* dep_job;         /* [D] the key; strictly ascending inside a job's list (deps is a map: the keys are distinct) */
  const uint64_t* dep_delay_sec;   /* [D] pair::second (CtldPublicDefs.cpp:151); the dependency type is not read by update */
  const uint8_t* array_parent;     /* [J] job->IsArrayParent() (:1397); NULL = none */
  const uint8_t* ap_flags;         /* [J] CNS_GATE_AP_*; read where array_parent[j] */
  const int64_t* ap_deadline_sec;  /* [J] parent_job_->deadline_time              Array.cpp:246 */
  const uint64_t* ap_running;      /* [J] RunningChildCount()                     Array.cpp:255 */
  const uint64_t* ap_run_limit;    /* [J] ArrayUtil::EffectiveRunLimit(array_spec) Array.cpp:253-254 */
} cns_gate_jobs;

/* What try_dequeue_bulk handed out (:1357), in queue order. */
typedef struct cns_gate_events {
  uint64_t num_events;
  const uint32_t* dependent_job_id;  /* [E] DependencyEvent::dependent_job_id (:1362) */
  const uint32_t* dependee_job_id;   /* [E] DependencyEvent::dependee_job_id  (:1364) */
  const int64_t* event_sec;          /* [E] DependencyEvent::event_time       (:1365) */
} cns_gate_events;

/* Results, caller-allocated. */
typedef struct cns_gate_out {
  uint8_t* code;          /* [J] cns_gate_code */
  uint32_t* pending;      /* [J] room; the first *num_pending entries are written: the rows with CNS_GATE_OK / _OK_ARRAY_PARENT, ascending */
  uint64_t* num_pending;
  int64_t* ready_sec;     /* [J] ready_time after the events; may be NULL */
  uint8_t* dep_erased;    /* [D] 1 where an event erased the entry (the caller removes those); may be NULL */
  uint64_t* counts;       /* [16] jobs per code; may be NULL */
  uint64_t* ev_stats;     /* [3] events applied, ignored for no such pending job, ignored for no such dependency (repeats included); may be NULL */
} cns_gate_out;

/* ev == NULL or num_events == 0: no events.  kernel_ms (may be NULL): HIP-event time of the call's kernels. */
int cns_gate_pending(cns_handle* h, int64_t now_sec, const cns_gate_jobs* jobs, const cns_gate_events* ev, const cns_gate_out* out,
                     double* kernel_ms);
/* Where the kernels' paths change: jobs per workgroup; the most dependency entries a single lane walks (a longer list is the whole
 * wave's); the per-wave counts one step of the compaction's scan takes (a queue of more than scan_span * 64 jobs carries a prefix from
 * one step into the next). */
int cns_gate_shape(uint32_t* job_chunk, uint32_t* lane_max_deps, uint32_t* scan_span);

#ifdef __cplusplus
}
#endif
#endif /* CRANE_GPU_PENDING_GATE_H_ */
