/*
 * crane_gpu_probe/probe.h — what-if start-time probes against the final state of a scheduling cycle.
 * (A directory of its own beside crane_gpu/: that directory's file list is the pinned ABI 4 surface, tests/test_abi.py; this header
 * adds calls and changes no existing struct, so CNS_ABI_VERSION stays 4.)
 *
 * After a successful cycle (cns_select / cns_run_resident) the model of that cycle is still resident in HBM: every node's
 * time map, every (partition, node) cost, the front summaries.  A PROBE is a job in the form of cns_job_soa that is asked
 * against that state: "when and where would this job run if it were submitted now?" — a submission dry run, an expected
 * start for the jobs beyond cns_config::scheduled_batch_size, an admission front end that wants to say "this can never
 * run here".  The reference has no such call (its only way to the answer is another NodeSelect with the job appended,
 * src/CraneCtld/JobScheduler.cpp:6507-6836, which also commits the job).
 *
 * Semantics.  For every probe, independently of every other probe of the call, the result is bit for bit what the cycle
 * would have written for it — start_sec, reason and, per node, (node_idx, ntasks, cpu_raw, mem, core_lo, core_hi, core_w2,
 * core_w3, gres), records sorted by node index — had it been handed to the ordered loop directly behind the last job that
 * loop took (JobScheduler.cpp:6743), at the cycle's `now`; and NOTHING IS COMMITTED:
 *   - the model is read-only under a probe call: costs, time maps, front summaries, the cycle's own results (cns_download,
 *     cns_device_results) and cns_get_timing are unchanged after it; the same call twice gives the same answer; permuting the
 *     probes permutes the answers;
 *   - probes are never cut by scheduled_batch_size (they are questions, not the queue); with a batch limit the state they see
 *     is the state after the jobs the loop took;
 *   - `skip` != 0 -> CNS_REASON_SKIPPED; partition >= num_partitions -> CNS_REASON_PARTITION_NOT_FOUND; `reservation` as in a
 *     cycle (the virtual partition of an active reservation, else CNS_REASON_RESERVATION_NOT_FOUND); a probe into a refused
 *     group of partitions (cns_get_partition_status) -> CNS_REASON_ENGINE_REFUSED; a later start carries "Resource Reserved" /
 *     "Resource" / "Priority" exactly as JobScheduler.cpp:6797-6831; a node whose time map has reached
 *     max_job_num_per_node entries at the END of the cycle is skipped (:6194);
 *   - every job shape the cycle serves: node_num >= 1, ntasks > node_num, exclusive, include / exclude lists, fractional
 *     cpus, GRES typed / untyped, core ids up to 255, partitions that share nodes (a probe sees the slots of its own
 *     partition, the node's one time map, its own partition's cost), partitions of every width the engine serves — the state
 *     has the same layout whichever selection kernel produced it;
 *   - a cycle over an EMPTY queue is a cycle: probes behind it are answered against the snapshot (running jobs, reservations) as
 *     cns_set_nodes / cns_set_running left it; a probe into a partition the last cycle had no job for sees that partition's
 *     snapshot, never what an earlier cycle on the handle left there;
 *   - the table is validated like a queue (cns_upload_jobs): a request for a GRES class the layout does not define refuses the
 *     whole call with CNS_ERR_INVALID_ARG ("probe job requests an undefined GRES class") and writes nothing — the reference
 *     would ignore such a request.
 *
 * State.  CNS_ERR_STATE before a successful run and after anything that invalidates it (cns_set_nodes,
 * cns_set_reservations, cns_set_running, cns_upload_jobs without a run).  After a cycle that ran cns_select_preempt with
 * cns_preempt_soa::enabled set: CNS_ERR_UNSUPPORTED — a probe that may itself preempt is a different question (it would have
 * to release resources in a state it must not touch) and is not built.  Several devices (cns_group_*): probe the device that
 * owns the partition through cns_group_handle(g, cns_group_device_of_partition(g, p)), with the partition indices of that
 * device's share; the group has no probe call of its own.
 *
 * Ownership, errors, threading: as in node_select.h.  The caller keeps its arrays (they are copied before the call returns);
 * the calls never throw, return 0 or a negative cns_status, and belong to the handle's one caller thread.  The probe table, its
 * results and its scratch live in device buffers of their own: the cycle's job table and packed result buffer survive.
 * There is no CPU fallback.
 */
#ifndef CRANE_GPU_PROBE_H_
#define CRANE_GPU_PROBE_H_

#include <stdint.h>

#include "../crane_gpu/node_select.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Q = probes->num_jobs probes in one call; out: caller-allocated as for cns_select (place_capacity >= sum(node_num), core_w2 /
 * core_w3 required when a node of the snapshot has a core id above 127).  num_jobs == 0 is CNS_OK and writes nothing.
 * kernel_ms (may be NULL): HIP-event time of the probe kernel. */
int cns_probe(cns_handle* h, const cns_job_soa* probes, cns_placement_soa* out, double* kernel_ms);

/* Split form (measurements: the timed region starts with the probes resident in HBM). */
int cns_probe_upload(cns_handle* h, const cns_job_soa* probes);       /* validates like cns_upload_jobs, packs the records on the device */
int cns_probe_run_resident(cns_handle* h, double* kernel_ms);          /* may be repeated: every run answers the uploaded probes anew */
int cns_probe_download(cns_handle* h, cns_placement_soa* out);

/* The constants at which k_probe changes path, as this build has them (tests/probe_seams.py puts a case on each).  Needs no handle
 * and no GPU; out == NULL -> CNS_ERR_INVALID_ARG. */
typedef struct cns_probe_shape_info {
  uint32_t block;          /* lanes of a probe's workgroup: the candidate walk strides over a partition's slots, the emit loop over
                              node_num, in steps of this */
  uint32_t dip_cpu_sat;    /* a dip's whole cpus (rounded up) saturate here: a saturated field refuses nothing */
  uint32_t dip_mem_sat;    /* ... its GiB (rounded up) */
  uint32_t dip_gres_sat;   /* ... its slots of one GRES class */
  uint32_t gres_classes;   /* classes / names a dip and a request are compared over */
  uint32_t gres_names;
  uint32_t max_types;      /* distinct res_total records of a snapshot (CNS_MAX_NODE_TYPES): one lane per type */
  uint32_t heap_ent_bytes; /* one entry of a workgroup's heap scratch */
  uint32_t loff_clamp;     /* a time limit of this many seconds or more reaches every dip (dips are 32 bits of seconds after now) */
  uint32_t pad;
  uint64_t scratch_cap;    /* bytes of heap scratch a call may take: min(widest partition, widest node_num) + 1 entries per resident
                              workgroup, fewer workgroups where that would exceed it, never fewer than one.  The environment variable
                              CNS_PROBE_SCRATCH_CAP (bytes) lowers it, never raises it; a value that does not begin with a digit is
                              ignored. */
} cns_probe_shape_info;
int cns_probe_shape(cns_probe_shape_info* out);

/* Test hooks, beside cns_debug_get_costs.  cns_debug_get_probe_plan: the workgroups and the heap entries per workgroup of the last
 * cns_probe_run_resident (0, 0 where no probe reached a walk).  cns_debug_get_dips: per (partition, node) slot, [len(part_nodes)] in
 * the order of cns_debug_get_costs, the dip the last cycle left: seconds after now (0xFFFFFFFF: none) | whole cpus << 16 | GiB |
 * a nibble per GRES class. */
int cns_debug_get_probe_plan(cns_handle* h, uint64_t* grid, uint32_t* stride);
int cns_debug_get_dips(cns_handle* h, uint32_t* dip_t, uint32_t* dip_cm, uint32_t* dip_g);

#ifdef __cplusplus
}
#endif
#endif /* CRANE_GPU_PROBE_H_ */
