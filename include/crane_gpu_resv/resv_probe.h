/*
 * crane_gpu_resv/resv_probe.h — reservation what-ifs: which nodes could a new reservation take, and how soon?
 * (A directory of its own beside crane_gpu/, as crane_gpu_probe/: that directory's file list is the pinned ABI 4 surface,
 * tests/test_abi.py; this header adds calls and changes no existing struct, so CNS_ABI_VERSION stays 4.)
 *
 * The reference answers this inside JobScheduler::CreateResv_ (src/CraneCtld/JobScheduler.cpp:4375-4441): a serial walk over
 * the candidate nodes under the running-job mutex and the resource-reduce lock, per node every running job's end time
 * (:4391-4400) and every reservation on the node (:4403-4410), the first `node_num` nodes that pass are taken (:4416).  It says
 * yes or no for the ONE start time of the request.  Here Q such requests are answered in one call, each either at its start
 * time or — what the reference cannot say — at the EARLIEST start at which it fits; nothing is created.
 *
 * Node state (cns_resvq_set_state) is per NODE, not per scheduler slot, as in the reference (:4391-4410 read CranedMeta):
 *   latest_end[n]  max end_sec over the running allocations on node n, whichever reservation the job runs in and whether or
 *                  not the node is schedulable (INT64_MIN without an allocation);
 *   resv[n]        (start_sec, end_sec) of every reservation that lists n, expired ones included (:4405 tests overlap only).
 *
 * A candidate of a query evaluated at start t with duration d, end = t + d (saturating at INT64_MAX), gets the code
 *   CNS_RESVQ_NOT_FOUND (3)  node index >= num_nodes (:4385-4388); never an error;
 *   CNS_RESVQ_RUNNING   (1)  latest_end > t (:4395) — tested first, as the reference does;
 *   CNS_RESVQ_RESERVED  (2)  a reservation of the node with st < end && ed > t (:4405);
 *   CNS_RESVQ_FREE      (0)  otherwise.
 * k = node_num, or the list length when node_num == 0 (:4357-4358; "not found" entries count).  EVERY candidate is coded; the
 * reference stops its walk at the k-th free node (:4416), so its nodes_conflicted / nodes_not_found are the prefix of this
 * answer up to that node — the whole list is a superset and is what an operator wants to see.
 *
 *   find_earliest == 0: t = start_sec.  status OK iff num_free >= k.
 *   find_earliest != 0: t = the least t in [start_sec, INT64_MAX) at which at least k candidates are free for [t, t + d).
 *                       (Not monotone in t: a node free now can run into a future reservation later.  The free count rises
 *                       only at start_sec, at a candidate's latest_end and at the end of a reservation on a candidate.)
 *                       No such t (fewer than k candidates found, or a needed node never frees: an end at INT64_MAX is never
 *                       reached): NOT_ENOUGH, reported at start_sec.
 *   start_sec + duration_sec <= now_sec: status IN_THE_PAST (:4323) for that query — start 0, num_free 0, its codes all 0,
 *                       nothing chosen; the other queries are answered.
 *
 * Errors: CNS_ERR_STATE before cns_set_nodes / cns_resvq_set_state (cns_set_nodes invalidates the state); CNS_ERR_INVALID_ARG
 * for a missing array, a candidate list that names a node twice, duration_sec <= 0, start_sec + duration_sec beyond INT64_MAX,
 * offsets that decrease, or result arrays that are too small; CNS_ERR_UNSUPPORTED above the limits: 2^31-1 candidates in one
 * call, and 2^26 INTERVALS in one call (an earliest-start query costs, per found candidate, one interval plus one per
 * reservation on the node; queries at a given start cost none).  Never a device fault.
 *
 * The calls read and write device buffers of their own: a cycle (cns_select ...) or a cns_probe before or after them behaves
 * exactly as without them.  Ownership, errors, threading: as in node_select.h — the caller keeps its arrays, the calls never
 * throw and belong to the handle's one caller thread.  There is no CPU fallback.
 */
#ifndef CRANE_GPU_RESV_PROBE_H_
#define CRANE_GPU_RESV_PROBE_H_

#include <stdint.h>

#include "../crane_gpu/node_select.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef enum cns_resvq_status { CNS_RESVQ_OK = 0, CNS_RESVQ_NOT_ENOUGH = 1, CNS_RESVQ_IN_THE_PAST = 2 } cns_resvq_status;
typedef enum cns_resvq_code { CNS_RESVQ_FREE = 0, CNS_RESVQ_RUNNING = 1, CNS_RESVQ_RESERVED = 2, CNS_RESVQ_NOT_FOUND = 3 } cns_resvq_code;

typedef struct cns_resvq_soa {
  uint64_t num_queries;
  const int64_t* start_sec;       /* [Q] may lie before now_sec (:4326)                                   */
  const int64_t* duration_sec;    /* [Q] > 0                                                              */
  const uint32_t* node_num;       /* [Q] 0 = all of the list (:4357-4358)                                 */
  const uint64_t* cand_offsets;   /* [Q+1] CSR into cand_nodes                                            */
  const uint32_t* cand_nodes;     /* the candidates in the caller's order (:4383); distinct inside a list */
  const uint8_t* find_earliest;   /* [Q] NULL = all 0                                                     */
} cns_resvq_soa;

/* Results, caller-allocated. */
typedef struct cns_resvq_out {
  uint64_t code_capacity;     /* >= cand_offsets[Q]                                                       */
  uint64_t chosen_capacity;   /* >= sum over the queries of min(k, list length)                           */
  uint8_t* status;            /* [Q] cns_resvq_status                                                     */
  int64_t* start_sec;         /* [Q] the start the answer holds for; 0 unless status is OK                */
  uint32_t* num_free;         /* [Q] free candidates of the whole list at the evaluated start             */
  uint8_t* code;              /* [code_capacity] cns_resvq_code per candidate, in list order              */
  uint64_t* chosen_offsets;   /* [Q+1] CSR into chosen_nodes                                              */
  uint32_t* chosen_nodes;     /* the first k free candidates in list order; empty unless status is OK     */
} cns_resvq_out;

/* After cns_set_nodes (only its num_nodes is used).  running / resv: the tables of cns_set_running / cns_set_reservations
 * (alloc_node, end_sec, start_sec, the CSR offsets; the resource columns are not read); either may be NULL: none. */
int cns_resvq_set_state(cns_handle* h, const cns_running_soa* running, const cns_resv_soa* resv);
/* num_queries == 0 is CNS_OK and writes nothing.  kernel_ms (may be NULL): HIP-event time of the call's kernels. */
int cns_resvq_run(cns_handle* h, int64_t now_sec, const cns_resvq_soa* q, cns_resvq_out* out, double* kernel_ms);
/* The constants at which the device code changes path, for tests that put a case on each; no handle, any pointer may be NULL.
 * pick_block: candidates one step of the pick kernel takes (a list longer than that carries a count between its steps);
 * pick_grid: workgroups of the pick kernel (more queries than that: a workgroup takes several); sort_tile: event times per tile of
 * the sort; scan_span: tiles one step of the sort's scan takes (more than scan_span * sort_tile event times: a carry between the
 * steps).  Always CNS_OK. */
int cns_resvq_shape(uint32_t* pick_block, uint32_t* pick_grid, uint32_t* sort_tile, uint32_t* scan_span);

#ifdef __cplusplus
}
#endif
#endif /* CRANE_GPU_RESV_PROBE_H_ */
