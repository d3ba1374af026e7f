/*
 * crane_gpu_valid/validity.h — can each job of a batch EVER run in the partition it names, and on how many nodes?
 * (A directory of its own beside crane_gpu/, as crane_gpu_probe/ and crane_gpu_resv/: that directory's file list is the pinned
 * ABI 4 surface, tests/test_abi.py; this header adds calls and changes no existing struct, so CNS_ABI_VERSION stays 4.)
 *
 * The reference answers this in JobScheduler::CheckJobValidity (src/CraneCtld/JobScheduler.cpp:7224-7377): a test of the job's
 * total request against the partition's total (:7283-7297), then a serial walk over every node of the partition, each under
 * that node's exclusive lock (:7353-7365).  It runs once per submission on the RPC thread (:3458) and once per recovered pending
 * job at start-up (:371).  Here J jobs are answered in one call, against the node table of the last cns_set_nodes (and, for
 * the reservation checks, of the last cns_set_reservations: without one num_resv is 0).
 *
 * It is NOT the test a scheduling cycle makes (cns_select's feasibility):
 *   - the walk tests req_node_res_view + req_task_res_view, i.e. ONE task (:7356), not ntasks_per_node_min tasks;
 *   - it tests counts only (PublicHeader.cpp:619-646): no core ids, no slot identity;
 *   - it tests against res_total of every node the partition lists (:7354-7357), alive, drained or neither: CranedDown leaves
 *     res_total as it is (CranedMetaContainer.cpp:83-122), so cns_node_soa::schedulable is not read;
 *   - the partition's total is res_total_inc_dead (:7284), the sum over every listed node (CranedMetaContainer.cpp:364-391).
 *
 * Per job the code is the FIRST failing check, in the reference's order:
 *   CNS_VALID_BAD_REQUEST          node_num == 0, ntasks < node_num, or a 64-bit overflow in node_mem*node_num + task_mem*ntasks,
 *                                  node_cpu*node_num + task_cpu*ntasks (:7156-7157), node_mem + task_mem, node_cpu + task_cpu
 *                                  (:7356): the reference's arithmetic is undefined there; such a job is never OK
 *   CNS_VALID_ZERO_MEM             node_mem*node_num + task_mem*ntasks == 0 (:7262; req_total_res_view is composed at :7156-7157)
 *   CNS_VALID_ZERO_CPU             task_cpu_raw == 0 (:7266)
 *   CNS_VALID_PARTITION_NOT_FOUND  partition >= num_partitions.  The partition is looked at for reservation jobs too: :7278 and
 *                                  :7354 use job->partition_id whatever the reservation is
 *   CNS_VALID_REFUSED              NOT a result of the reference: the partition lists a node flagged cns_node_soa::unsupported
 *                                  (its res_total is not expressible here) — ask the CPU code.  Only the jobs of that partition get
 *                                  it; sharing a node with such a partition refuses nobody here
 *   CNS_VALID_NO_RESOURCE          req_total <= partition total fails (:7283; PublicHeader.cpp:648-659 and :57-69): cpu and mem
 *                                  compared raw (mem_sw is not tested, :649-650); per requested GRES name gres_total*node_num <= the
 *                                  partition's slot count of the name, and the name must exist (:653-654,:59); per specified class
 *                                  the class must exist in the partition and gres_spec*node_num <= its slot count (:62-66)
 *   CNS_VALID_NODE_NUM             node_num > number of nodes the partition lists (:7299)
 *   CNS_VALID_RESV_NOT_FOUND       reservation != CNS_RESV_NONE and >= num_resv (:7308).  Existence only, active or not
 *   CNS_VALID_RESV_NODE            an included node is not a node of the reservation (:7338-7349)
 *   CNS_VALID_NOT_ENOUGH_NODES     eligible < node_num (:7368)
 *   CNS_VALID_OK                   otherwise (:7376)
 *
 * eligible[j] = the number of nodes n the job's partition lists with (:7356-7361)
 *   node + task request <= res_total[n] by PublicHeader.cpp:619-646: cpu raw (:620) and mem (:621); per requested name the name is
 *     present on the node (:626-627) and gres_total <= the node's slots of that name over all its types (:639-642); per specified class
 *     the class is present on the node (:633-634) and gres_spec <= its slots (:635);
 *   the include list is empty or names n (:7358-7359);
 *   the exclude list does not name n (:7360-7361).
 * It is written for every job whose code is NOT_ENOUGH_NODES or OK, else 0.  The reference stops counting at node_num (:7364): its
 * number is min(eligible, node_num).  The FULL count is reported here: it is what an operator wants to see.
 *
 * Input rules.  cns_node_soa::schedulable is not read.  A list entry >= num_nodes, or one that names a node outside the partition,
 * matches nothing (the reference holds names); for CNS_VALID_RESV_NODE such an entry is "not a node of the reservation".  Lists are
 * sets: a node named twice inside one list is CNS_ERR_INVALID_ARG.  A zero count in gres_total / gres_spec is no entry at all (as for
 * the cycle, INTEGRATION.md 3: the reference would still ask for the name / type to exist).  A gres_spec count of a class the layout
 * does not define asks for a class no partition has: CNS_VALID_NO_RESOURCE.  A node whose cpu_total_raw is negative is
 * CNS_ERR_INVALID_ARG; the partition's sums saturate at INT64_MAX / UINT64_MAX.
 * skip, exclusive, time_limit_sec and ntasks_per_node_min / _max are NOT read (those arrays may be NULL).
 *
 * With the caller (fields the job table does not carry): the time limit (:7225), the array spec (:7229-7259), the deadline (:7271),
 * and the reservation's partition / account / user lists (:7317-7336).
 *
 * Errors: CNS_ERR_STATE before a cns_set_nodes that returned CNS_OK (a snapshot of which the cycle serves NO partition is refused by
 * cns_set_nodes with CNS_ERR_UNSUPPORTED and leaves no node table: ask the CPU code); CNS_ERR_INVALID_ARG for a missing array, list offsets that decrease or a node twice in
 * one list; CNS_ERR_UNSUPPORTED for more than 2^32 - 16 jobs in one call.  Never a device fault.  num_jobs == 0 is CNS_OK and writes
 * nothing.  The call reads and writes device buffers of its own (derived tables built at the first call after cns_set_nodes /
 * cns_set_reservations): a cycle, a cns_probe or a cns_resvq_run before or after it behaves exactly as without it.  Ownership, errors,
 * threading: as in node_select.h — the caller keeps its arrays, the call never throws and belongs to the handle's one caller thread.
 * There is no CPU fallback.
 */
#ifndef CRANE_GPU_VALIDITY_H_
#define CRANE_GPU_VALIDITY_H_

#include <stdint.h>

#include "../crane_gpu/node_select.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef enum cns_valid_code {
  CNS_VALID_OK = 0,
  CNS_VALID_BAD_REQUEST = 1,
  CNS_VALID_ZERO_MEM = 2,             /* ERR_INVALID_PARAM, :7264     */
  CNS_VALID_ZERO_CPU = 3,             /* ERR_INVALID_PARAM, :7268     */
  CNS_VALID_PARTITION_NOT_FOUND = 4,
  CNS_VALID_REFUSED = 5,
  CNS_VALID_NO_RESOURCE = 6,          /* ERR_NO_RESOURCE, :7296       */
  CNS_VALID_NODE_NUM = 7,             /* ERR_INVALID_NODE_NUM, :7304  */
  CNS_VALID_RESV_NOT_FOUND = 8,       /* ERR_INVALID_PARAM, :7312     */
  CNS_VALID_RESV_NODE = 9,            /* ERR_INVALID_PARAM, :7347     */
  CNS_VALID_NOT_ENOUGH_NODES = 10     /* ERR_NO_ENOUGH_NODE, :7373    */
} cns_valid_code;

/* Results, caller-allocated. */
typedef struct cns_validity_out {
  uint8_t* code;       /* [J] cns_valid_code                                                        */
  uint32_t* eligible;  /* [J] nodes of the partition that pass the walk's test (the full count)     */
} cns_validity_out;

/* After cns_set_nodes.  kernel_ms (may be NULL): HIP-event time of the walk kernel (the derived tables, built at the first call after
 * cns_set_nodes, are not in it). */
int cns_validate_jobs(cns_handle* h, const cns_job_soa* jobs, const cns_validity_out* out, double* kernel_ms);
/* The tile sizes of the walk kernel: node records staged per step, jobs per workgroup (where its paths change). */
int cns_validate_shape(uint32_t* node_tile, uint32_t* job_chunk);

#ifdef __cplusplus
}
#endif
#endif /* CRANE_GPU_VALIDITY_H_ */
