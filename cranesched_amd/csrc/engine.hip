// Host side of the C ABI (include/crane_gpu/node_select.h): validation, SoA packing, HBM residency,
// kernel launches and timing.  No scheduling decision is taken on the host and there is no CPU
// fallback: without a usable HIP device cns_create fails with CNS_ERR_NO_DEVICE.
//
// Reference counterparts of the host-side packing (all in src/CraneCtld/JobScheduler.cpp):
//   split of the pending queue by partition            :6516-6530
//   partition -> node list, skip !alive || drain       :6569-6617
//   running jobs' per-node allocations                 :6681-6709
//   BasicPriority truncation to ScheduledBatchSize     JobScheduler.h:185-200
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <set>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/crane_gpu/node_select.h"
#include "../../include/crane_gpu/preempt.h"
#include "../../include/crane_gpu/priority.h"
#include "../../include/crane_gpu_probe/probe.h"
#include "../../include/crane_gpu_resv/resv_probe.h"
#include "../../include/crane_gpu_valid/validity.h"
#include "../../include/crane_gpu_commit/commit_check.h"
#include "../../include/crane_gpu_submit/submit_limits.h"
#include "../../include/crane_gpu_gate/pending_gate.h"
#include "../../include/crane_gpu_usage/usage.h"
#include "../../include/crane_gpu_running/running.h"
#include "../../include/crane_gpu_running/running_preempt.h"
#include "../../include/crane_gpu_running/running_attrs.h"
#include "../../include/crane_gpu_amend/running_amend.h"
#include "../../include/crane_gpu/run_limits.h"
#include "../../include/crane_gpu/steps.h"
#include <limits>
#include "engine_params.h"
#include <rccl/rccl.h>          // several devices: group_host.inc (the engine library links RCCL)
#include "select_kernels.hip"  // single translation unit: kernels + their launches (no -fgpu-rdc needed)
#include "sort_kernels.inc"    // the stable pair sort and the ordered scan of per-wave counts that every later kernel file builds on
#include "priority_kernels.hip"
#include "limits_kernels.hip"
#include "steps_kernels.hip"
#include "probe_kernel.inc"    // k_probe: what-if probes against the final state of a cycle (include/crane_gpu_probe/probe.h)
#include "resvq_kernels.inc"  // reservation what-ifs: which nodes, how soon (include/crane_gpu_resv/resv_probe.h)
#include "valid_kernels.inc"  // can each job of a batch ever run in its partition (include/crane_gpu_valid/validity.h)
#include "commit_kernels.inc" // the commit loop's resource-changed and preempted-alive checks (include/crane_gpu_commit/commit_check.h)
#include "submit_kernels.inc" // the submit limits over a batch of submissions (include/crane_gpu_submit/submit_limits.h)
#include "usage_kernels.inc"  // releases and charges of a batch of jobs on the usage tables (include/crane_gpu_usage/usage.h)
#include "gate_kernels.inc"   // the dependency-event drain and Phase 1 in front of a cycle (include/crane_gpu_gate/pending_gate.h)
#include "running_kernels.inc" // the running set kept on the device between two cycles: retire, admit, rebuild (include/crane_gpu_running/running.h)
#include "running_preempt_kernels.inc" // a cycle with preemption on that set: the entry index, the job -> entries CSR, the marks and the end patch (include/crane_gpu_running/running_preempt.h)
#include "running_attrs_kernels.inc" // the attribute columns beside that set, the per-row sums and the running side of the sorter taken from them (include/crane_gpu_running/running_attrs.h)
#include "running_amend_kernels.inc" // a running job's end time changed on that set: the end column and the per-slot end times (include/crane_gpu_amend/running_amend.h)
#include "jobs_host.inc"       // the host pass of cns_upload_jobs (no HIP in there: also compiled by the CPU tests)
#include "plan_host.inc"       // the launch plan of a cycle: which kernel serves which partitions (no HIP in there either)
#include "csr_host.inc"        // the CSR rules of the callers' lists: offsets, sorted lists without a repeat (no HIP in there either)
#include "snapshot_host.inc"   // the layout of a snapshot: groups, refusals, slots, reservations, node types, running entries (no HIP in there either)
#include "gate_check_host.inc" // the input rules of cns_gate_pending (no HIP in there either)
#include "acct_space_host.inc" // the record space the run limits, the submit limits and the usage tables address, its account chains and key ranges (no HIP in there either)
#include "limits_check_host.inc" // the input rules of cns_set_run_limits / cns_upload_limit_jobs (no HIP in there either)
#include "submit_check_host.inc" // the input rules of cns_set_submit_limits / cns_check_submissions (no HIP in there either)
#include "usage_check_host.inc" // the input rules of cns_usage_set_tables / cns_usage_apply (no HIP in there either)
#include "running_check_host.inc" // the input rules of cns_running_seed / cns_running_advance (no HIP in there either)
#include "running_amend_check_host.inc" // the input rules of cns_running_amend_ends (no HIP in there either)
#include "preempt_host.inc"    // the host side of a cycle with preemption: who may preempt, the buffer plan, the running side, the fold of the results (no HIP in there either)
#include "running_preempt_check_host.inc" // the input rules of cns_running_select_preempt (no HIP in there either)
#include "running_attrs_check_host.inc" // the input rules of the calls of running_attrs.h (no HIP in there either)
#include "probe_plan_host.inc" // the launch plan of k_probe: workgroups, heap stride, scratch bytes under the cap (no HIP in there either)
#include "sort_host.inc"       // the arithmetic of the pair sort: passes, tiles, histogram bytes (no HIP in there either)
#include "resvq_passes.inc"    // the radix passes over the segment numbers of cns_resvq_run's sort (no HIP in there either)
#include "buf_slots.h"         // the slots of cns_engine's per-feature buffer sets

using namespace cns;

namespace {

// Widest snapshots served.  A partition that shares no node and is wider than k_wide's widest tile (65 536 slots), and a group of
// partitions sharing nodes that is wider than k_mem's ordinary row masks (143 360 slots), run on k_giant (launch_giant: the home
// workgroup's sequential protocol plus helper workgroups that scan stripes of the slots); where the helpers' co-residency cannot be
// proven, on k_mem — its 5-word masks up to 143 360 slots, the giant instantiation's 19-word masks above.  Above these limits:
// CNS_PART_REFUSED_WIDTH for that partition / group only.
constexpr u32 kGiantPartSlots = 262144;   // one partition that shares no node (and one reservation's virtual partition)
constexpr u32 kGiantGroupSlots = 524288;  // a group of partitions that share nodes (ALL over 262 144 nodes + subsets that cover it once more)
static_assert(kGiantPartSlots <= kGiantGroupSlots && kGiantGroupSlots <= w8::WideInfo::giant_mem_slots, "k_mem's giant masks hold the widest group");
static_assert(w8::WideInfo::mem_slots >= w64::WideInfo::lanes * w64::WideInfo::npl_max, "k_wide's widest tile stays below k_mem's ordinary masks");
// the widest partition / group a snapshot may hold (cns_set_nodes refuses the others with CNS_PART_REFUSED_WIDTH), and its node types
const cns_snapshot::Caps kCaps{kGiantPartSlots, kGiantGroupSlots, CNS_MAX_NODE_TYPES};
static_assert(cns_snapshot::kNone == kNone && cns_snapshot::kTlCap == kTlCap && CNS_MAX_NODE_TYPES == CNS_MAX_NODE_TYPES_DEV, "snapshot_host.inc: the kernels' constants");

std::string g_create_error;

struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }
  hipError_t ensure(size_t bytes) {
    if (bytes <= cap && p) return hipSuccess;
    if (p) { (void)hipFree(p); p = nullptr; cap = 0; }
    size_t want = bytes ? bytes : 16;
    hipError_t e = hipMalloc(&p, want);
    if (e == hipSuccess) cap = want;
    return e;
  }
  void release() { if (p) { (void)hipFree(p); p = nullptr; cap = 0; } }
  template <class T> T* as() const { return static_cast<T*>(p); }
};

// Page-locked host staging for what cns_upload_jobs computes on the host (pre-set reasons, placement offsets, the grouped queue):
// a copy from a std::vector is a bounce through the runtime's own pinned buffer ON the calling thread; from here it is a DMA the
// thread does not wait for.  Grows by a quarter beyond the request (a queue that gains a few jobs per cycle re-pins nothing).
struct PinBuf {
  void* p = nullptr;
  size_t cap = 0;
  PinBuf() = default;
  PinBuf(const PinBuf&) = delete;
  PinBuf& operator=(const PinBuf&) = delete;
  ~PinBuf() { release(); }
  hipError_t ensure(size_t bytes) {
    if (bytes <= cap && p) return hipSuccess;
    if (p) { (void)hipHostFree(p); p = nullptr; cap = 0; }
    const size_t want = bytes ? bytes + bytes / 4 : 64;
    hipError_t e = hipHostMalloc(&p, want, hipHostMallocDefault);
    if (e == hipSuccess) cap = want;
    return e;
  }
  void release() { if (p) { (void)hipHostFree(p); p = nullptr; cap = 0; } }
  template <class T> T* as() const { return static_cast<T*>(p); }
};

// One uploaded cns_job_soa and its results.  The engine holds two: the cycle's queue (cns_engine::q) and the what-if probes against the
// cycle's final state (cns_engine::pt).  job_table.inc has the steps the two callers sequence.
struct JobTable {
  DevBuf raw[JR_COUNT];                                  // the caller's arrays as uploaded, the place offsets, the grouped table (buf_slots.h)
  DevBuf incl, excl, jtag, jobs, reason_init, results;   // node lists, member tags, the 64-dword records, the pre-set reasons, the packed results
  PinBuf h_place, h_grouped, h_reason, h_jtag;           // what the host pass computes; h_place [J + 1] also answers a download's place_offsets
  cns_jobs_host::ResOff ro{};                            // the sections of `results`
  u64 J = 0, Jg = 0, places = 0;                         // jobs, those that reach an ordered loop, placement records (set with ro: table_layout)
  std::vector<u32> job_part;                             // job (index of the caller's arrays) -> engine partition (kNone: not given to an ordered loop)
};

}  // namespace

struct cns_engine {
  cns_config cfg{};
  int device = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  hipStream_t stream2 = nullptr;                // second launch of a split cycle (the partitions that need k_select), beside the first
  hipEvent_t ev2[2] = {nullptr, nullptr};
  std::string err;

  // the snapshot (host copies, snapshot_host.inc): what cns_set_nodes, cns_set_reservations and cns_set_running derived from the caller's
  // arrays.  Each is replaced whole, and only by a call that passed validation.
  cns_snapshot::Layout lay;                   // partitions and groups, the slots of the real nodes
  cns_snapshot::ResvLayout rlay;              // ... extended by the reservations' virtual partitions: the slot list the device runs on
  cns_snapshot::RunLayout run;                // the running allocations grouped by slot (cns_select_preempt reads the entries)
  u32 num_cus = 0;                            // compute units of the device (0: unknown); k_wide needs one per workgroup, all resident at once
  std::vector<uint8_t> refused_probe;         // the statuses of the last cns_set_nodes call that computed them: a success, or the failure because EVERY
                                              // partition was refused (empty after any other failure)
  DevBuf d_slot_block, d_sib_off, d_sib, d_type_tag;
  GresDev gres{};
  bool have_nodes = false, have_jobs = false, have_run = false;

  DevBuf d_slot_total, d_slot_end, d_slot_type, d_rv_off, d_rv_start, d_rv_end, d_rv_res, d_first_resv, d_resv_se;
  // device buffers
  DevBuf d_part_off, d_slot_node, d_type_total, d_blocks, d_cost, d_fcpu,
      d_fmem, d_fcnt, d_dipt, d_dipcm, d_dipg, d_rn_off, d_rn_end, d_rn_res, d_heap, d_bfj, d_gupd, d_fault;
  DevBuf d_pj_off, d_params, d_prof, d_wide;
  JobTable q;                                   // the cycle's queue (cns_upload_jobs)
  u64 jobs_ordered = 0, algo_bytes = 0;
  u64 window_shaped = 0;   // jobs of the uploaded queue that a window of k_wide can decide: one node, one task per node, no GRES, no node lists, not exclusive
  u32 host_threads = 0;                         // cns_set_host_threads (0: CNS_HOST_THREADS, else up to 16)
  // what-if probes against the final state of the last cycle (probe_host.inc): a table and results of their own, and their scratch
  JobTable pt;
  DevBuf d_pb[PB_COUNT];
  u32 pkmax = 1;                                // the widest node_num of the probes that reach a walk
  bool have_probes = false, probes_answered = false;
  u64 probe_grid = 0; u32 probe_stride = 0;     // what the last cns_probe_run_resident launched (cns_debug_get_probe_plan)
  bool pre_call = false;                        // inside cns_select_preempt with preemption enabled
  bool run_preempt = false;                     // the last successful cycle was such a call (probes are not served behind it)
  double probe_ms = 0.0;
  // reservation what-ifs (resvq_host.inc): per-node tables, queries, event times and results in buffers of their own
  DevBuf d_rq[RQ_COUNT];
  u32 rq_N = 0;                                 // the node count the tables were built for
  std::vector<u32> rq_rv_cnt;                   // node -> reservations that list it
  bool rq_have = false;
  // the validity check of a batch of submissions (valid_host.inc): the caller's node arrays as cns_set_nodes got them, derived tables,
  // the call's job arrays and results in buffers of their own
  DevBuf d_vd[VD_COUNT];
  std::vector<i64> vd_cpu;
  std::vector<u64> vd_mem, vd_gres;
  std::vector<uint8_t> vd_unsup;
  std::vector<u32> vd_poff, vd_pnodes;          // the caller's partition lists: every listed node, schedulable or not
  u32 vd_V = 0;                                 // reservations of the device's membership table
  bool vd_tab_have = false, vd_rv_have = false; // the tables derived from the node arrays / from the reservations are built
  // the commit loop's checks behind a cycle (commit_host.inc): the call's events, job arrays and results in buffers of their own
  DevBuf d_cc[CC_COUNT];
  // the pending gate in front of a cycle (gate_host.inc): the call's jobs, events and results in buffers of their own
  DevBuf d_gate[GT_COUNT];
  cns_timing timing{};
  std::string last_kernel;
  i64 last_now = 0;
  std::vector<u64> part_jobs;                   // engine partition -> jobs of the uploaded queue that reach its ordered loop
  std::vector<uint8_t> pre_part;                // cycle with preemption: engine partition has a pending job whose qos may preempt
  DevBuf d_params2, d_pmap_a, d_pmap_b, d_wide_last;
  DevBuf d_params3, d_pmap_c, d_wide_mem;       // the serial-only launch of k_wide (groups wider than k_select's tile)
  DevBuf d_giant;                               // ... its GiantCtl blocks when it runs with helper workgroups (k_giant)
  DevBuf d_flen, d_tag_off, d_tag_base;         // ... its compact map lengths, and the slot range of every member partition of a group
  // several devices (group_host.inc): this engine's rank in a communicator, the all-gathered results of every rank
  void* comm = nullptr;                         // ncclComm_t
  u32 comm_nranks = 0, comm_rank = 0;
  DevBuf d_gather;
  double gather_ms = 0.0;
  u64 gather_bytes = 0;
  bool pass_waits = false;                      // a kernel the last pass launched has workgroups that wait for each other (k_wide, k_giant)
  u32 wide_retries = 0;                         // cycles that were re-run on k_pipe / k_select after a k_wide fault (lifetime of the handle)
  // MultiFactorPriority (priority_host.inc)
  DevBuf d_prio[PR_COUNT];
  double prio_ms = 0.0;
  u64 prio_bytes = 0;
  // run-limit admission (limits_host.inc)
  DevBuf d_lim[LM_COUNT], d_limpar[LP_COUNT];
  DevBuf d_step[ST_COUNT];  // step scheduler (steps_call.inc)
  // preemption (include/crane_gpu/preempt.h): what cns_set_running kept of the running set, and the cycle's tables
  std::set<void*> host_bufs;                    // page-locked host buffers handed out by cns_host_alloc
  bool pre_active = false;                      // the next run is a cycle with preemption (general path of k_select only)
  PreParams pre_params{};
  cns_preempt::Plan pre_plan{};                 // the sizes of d_pre for the cycle pre_params was bound for (preempt_host.inc)
  DevBuf d_pre[B_COUNT];
  bool lim_have_tables = false, lim_have_jobs = false, lim_have_run = false;
  bool lim_has_upl = false, lim_has_apl = false, lim_has_sel = false, lim_has_skip = false;
  cns_acct::Space lim_sp{}, sub_sp{}, use_sp{};  // the record space of each feature's tables as last set (acct_space_host.inc)
  u64 lim_J = 0, lim_sel_J = 0;
  std::vector<u32> lim_level;
  cns_limit_timing lim_timing{};
  // the submit limits over a batch of submissions (submit_host.inc): tables, the call's job arrays, items and results in buffers of their own
  DevBuf d_sub[SB_COUNT];
  bool sub_have = false, sub_has_upl = false, sub_has_apl = false, sub_has_uq = false, sub_has_aq = false, sub_has_g = false;
  u32 sub_max_set = 0, sub_max_cur = 0;         // the largest submit count of the tables as set / as the last call left them
  cns_gres_layout sub_lay{};
  cns_submit_timing sub_timing{};
  // releases and charges on the usage tables (usage_host.inc): three copies of the table, the call's rows, items and masks
  DevBuf d_use[US_COUNT];
  bool use_have = false, use_have_cur = false;  // tables set / a cns_usage_apply succeeded since
  cns_usage_timing use_timing{};
  // the running set kept on the device (running_host.inc): two copies of the ledger, the call's lists, counts and pairs, the per-slot
  // tables of the call (swapped with d_rn_off / d_rn_end / d_rn_res when it succeeded)
  DevBuf d_rl[RL_COUNT];
  bool rl_have = false;                         // a ledger is seeded (cns_set_running and a changed num_nodes drop it)
  bool rl_dev = false;                          // d_rn_* were built from the ledger: h->run holds no entries for them
  u32 rl_R = 0, rl_A = 0, rl_N = 0;             // its rows and allocations; the num_nodes it was seeded under
  u64 lay_gen = 0, rl_lay_gen = ~0ull;          // uploads of the snapshot so far; the one RL_NSOFF / RL_NS were derived from
  u32 rl_fan = 1;                               // slots of the node in most partitions
  cns_running_timing rl_timing{};
  cns_running_amend_timing am_timing{};         // the last cns_running_amend_ends (running_amend_host.inc)
  // a cycle with preemption on that set (running_preempt_host.inc): the sorted pairs of the rebuild the per-slot tables came from, the
  // index built from them, the call's lists and tables
  DevBuf d_rp[RP_COUNT];
  u32 rl_M = 0;                                 // (slot, allocation) pairs of that rebuild: the entries of the per-slot tables
  int rl_sorted_side = 0;                       // run_rebuild: which of RL_K0 / RL_K1 (RL_V0 / RL_V1) holds the sorted pairs
  bool rp_index = false;                        // RP_ENTJOB .. RP_RJENT describe the current per-slot tables
  bool rp_call = false;                         // RP_RJPRE, RP_RJEND, RP_ENTEND are those of a cns_running_select_preempt on that index
  bool run_preempt_rl = false;                  // the last successful cycle was such a call with preemption enabled (the admit step is served behind it)
  std::chrono::steady_clock::time_point pre_t0{};   // entry of the last cns_select_preempt / cns_running_select_preempt with preemption enabled
  cns_running_preempt_timing rp_timing{};       // ... what it spent in front of its cycle
  const i64* rn_end_bound = nullptr;            // the per-slot end times of the next run when they are not d_rn_end (the patched copy of such a call)
  // the attribute columns beside the ledger (running_attrs_host.inc): two copies, what a cycle boundary needs to carry them, the
  // per-row sums and the running side of cns_priority_order_resident
  DevBuf d_ra[RA_COUNT];
  bool ra_have = false;                         // the ledger carries columns (a plain seed / advance and whatever drops the ledger drop them)
  bool ra_sums = false;                         // RA_NODENUM, RA_CPU, RA_MEM, RA_SUMFLAG describe the current ledger
};

namespace {

int fail(cns_engine* h, int code, const std::string& msg) {
  if (h) h->err = msg; else g_create_error = msg;
  return code;
}
#define HIPCHK(h, call)                                                                         \
  do {                                                                                          \
    hipError_t _e = (call);                                                                     \
    if (_e != hipSuccess)                                                                       \
      return fail(h, CNS_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(_e));           \
  } while (0)

// after a failure nothing of the call is left in flight, and the message survives
void drain(cns_engine* h) {
  const std::string keep = h->err;
  if (hipSetDevice(h->device) == hipSuccess) (void)hipStreamSynchronize(h->stream);
  (void)hipGetLastError();
  h->err = keep;
}

// room for `bytes` in b, then the copy on the engine's stream (nothing to copy: a null source or no bytes)
int stage(cns_engine* h, DevBuf& b, const void* src, size_t bytes) {
  HIPCHK(h, b.ensure(bytes));
  if (bytes && src) HIPCHK(h, hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, h->stream));
  return 0;
}
template <class T>
int upload(cns_engine* h, DevBuf& b, const std::vector<T>& v) { return stage(h, b, v.data(), v.size() * sizeof(T)); }

using cns_jobs_host::align16;

#include "job_table.inc"   // the steps of a JobTable: check, lists_check, stage, route, layout, pack, reset, bind, download
#include "sort_call.inc"   // the launches of sort_kernels.inc: sort_pairs, sort_index_pairs, scan_counts

int build_gres(cns_engine* h, const cns_gres_layout& g) {
  GresDev d{};
  if (g.num_classes > CNS_MAX_GRES_CLASSES) return fail(h, CNS_ERR_INVALID_ARG, "gres.num_classes > 8");
  d.num_classes = g.num_classes;
  u64 seen = 0;
  for (u32 c = 0; c < g.num_classes; ++c) {
    if (g.class_name[c] >= CNS_MAX_GRES_NAMES) return fail(h, CNS_ERR_INVALID_ARG, "gres class name id >= 4");
    if (g.class_width[c] == 0 || g.class_shift[c] + g.class_width[c] > 64)
      return fail(h, CNS_ERR_INVALID_ARG, "gres class bit range outside 64-bit mask");
    u64 w = g.class_width[c] >= 64 ? ~0ull : ((1ull << g.class_width[c]) - 1ull);
    u64 m = w << g.class_shift[c];
    if (seen & m) return fail(h, CNS_ERR_INVALID_ARG, "gres classes overlap");
    seen |= m;
    d.class_mask[c] = m;
    d.class_name_packed |= (u32)g.class_name[c] << (4 * c);
    d.name_mask[g.class_name[c]] |= m;
    d.name_bytes[g.class_name[c]] |= 0xFFull << (8 * c);
  }
  h->gres = d;
  return 0;
}

// The A/B and test knobs of a run, read from the environment once per cns_run_resident: both passes of a retry see the same values,
// and there is no other getenv on the selection path.  Numbers: -1 = unset.
struct RunKnobs {
  cns_plan::Switch sw = cns_plan::Switch::Unset;   // CNS_SELECT_KERNEL (plan_host.inc: parse_kernel_switch)
  bool no_retry = false;                           // CNS_WIDE_NO_RETRY=1
  i64 inject_stall = -1, window = -1, tester_opt = -1, batch_post = -1, aux = -1;   // CNS_WIDE_INJECT_STALL, _WINDOW, _TESTER_OPT, _BATCH_POST, _AUX
  static RunKnobs read() {
    auto num = [](const char* name) { const char* e = getenv(name); return e ? (i64)(u32)strtoul(e, nullptr, 10) : (i64)-1; };
    RunKnobs k;
    k.sw = cns_plan::parse_kernel_switch(getenv("CNS_SELECT_KERNEL"));
    const char* nr = getenv("CNS_WIDE_NO_RETRY");
    k.no_retry = nr && nr[0] == '1';
    k.inject_stall = num("CNS_WIDE_INJECT_STALL"); k.window = num("CNS_WIDE_WINDOW"); k.tester_opt = num("CNS_WIDE_TESTER_OPT");
    k.batch_post = num("CNS_WIDE_BATCH_POST"); k.aux = num("CNS_WIDE_AUX");
    return k;
  }
};

// (the probes fill a block without knobs: no selection kernel runs there)
void fill_params(cns_engine* h, KParams& K, i64 now, const RunKnobs& kn = RunKnobs{}) {
  memset(&K, 0, sizeof K);
  K.num_nodes = h->lay.N; K.num_parts = h->rlay.P; K.num_slots = h->rlay.S; K.num_types = h->rlay.T;
  K.tl_cap = kTlCap;
  K.wide_cores = h->lay.wide_cores ? 1u : 0u;
  K.max_jobs_per_node = h->cfg.max_job_num_per_node;
  K.now = now;
  K.max_window = h->cfg.max_time_window_sec;
  if (kn.inject_stall >= 0) K.wide_inject_stall = (u32)kn.inject_stall + 1u;
  // jobs per pool exchange of k_wide's 64-wave build at most (wide_kernel.inc, "A WINDOW OF JOBS PER EXCHANGE"); 0 / 1: one job per exchange, as in
  // rounds 2-4 — and the kernel WITHOUT the window path is launched (k_wide<NPL, false>: the path's presence costs the single-job loops 8 %).
  // Unless CNS_WIDE_WINDOW says otherwise the QUEUE decides: windows for a queue that is (almost) all one-node jobs without GRES and node lists
  // (>= 95 %: C5 190 -> 185 ms, C2 / c5deep unchanged — where most jobs are backfilled the windows back off), none for a mix like C4's,
  // whose GRES backfills and multi-node jobs would close every window after two or three jobs (258 against 273 ms):
  // profiles/r05_ab_window_code_presence.txt, DESIGN.md 5.8.
  K.wide_window = (h->jobs_ordered != 0 && h->window_shaped * 100 >= h->jobs_ordered * 95) ? w64::kWJ : 0u;
  if (kn.window >= 0) K.wide_window = std::min<u32>((u32)kn.window, w64::kWJ);
  if (K.wide_inject_stall) K.wide_window = 0;
  K.wide_tester_opt = kn.tester_opt >= 0 ? (u32)kn.tester_opt : 1u;
  K.wide_aux = 0;   // (sized per launch: the plan's candidate)
  K.wide_batch_post = kn.batch_post >= 0 ? (u32)kn.batch_post : 1u;
  K.part_off = h->d_part_off.as<u32>();
  K.slot_node = h->d_slot_node.as<u32>();
  K.slot_total = h->d_slot_total.as<Res>();
  K.slot_end = h->d_slot_end.as<i64>();
  K.slot_type = h->d_slot_type.as<uint8_t>();
  K.rv_off = h->d_rv_off.as<u32>();
  K.rv_start = h->d_rv_start.as<i64>();
  K.rv_end = h->d_rv_end.as<i64>();
  K.rv_res = h->d_rv_res.as<Res>();
  K.first_resv = h->d_first_resv.as<i64>();
  K.resv_se = h->d_resv_se.as<i64>();
  K.num_real_parts = h->lay.P_real;
  K.type_total = h->d_type_total.as<Res>();
  K.blocks = h->d_blocks.as<char>();
  K.block_stride = kBlockStride;
  K.cost = h->d_cost.as<double>();
  K.f_cpu = h->d_fcpu.as<int>();
  K.f_mem = h->d_fmem.as<u32>();
  K.f_cnt = h->d_fcnt.as<u64>();
  K.dip_t = h->d_dipt.as<u32>(); K.dip_cm = h->d_dipcm.as<u32>(); K.dip_g = h->d_dipg.as<u32>();
  if (h->lay.shared) { K.f_len = h->d_flen.as<u32>(); K.tag_off = h->d_tag_off.as<u32>(); K.tag_base = h->d_tag_base.as<u32>(); }
  K.rn_off = h->d_rn_off.as<u32>();
  K.rn_end = h->rn_end_bound ? h->rn_end_bound : h->d_rn_end.as<i64>();
  K.rn_res = h->d_rn_res.as<Res>();
  K.pj_off = h->d_pj_off.as<u64>();
  table_bind(h, h->q, K);
  K.heap = h->d_heap.as<HeapEnt>();
  K.bf_j = h->d_bfj.as<u32>();
  K.g_upd = h->d_gupd.as<UpdRec>();
  K.fault = h->d_fault.as<u32>();
  K.prof = h->d_prof.as<u64>();
  K.wide_ctl = h->d_wide.as<char>();
  K.general_only = h->pre_active ? 1u : 0u;
  K.serial_only = 0;
  K.giant_ctl = nullptr; K.giant_nh = 0; K.pad_gnh = 0;
  K.pre = h->pre_active ? h->pre_params : PreParams{};
  K.gres = h->gres;
  if (h->lay.shared) {
    K.slot_block = h->d_slot_block.as<u32>(); K.sib_off = h->d_sib_off.as<u32>(); K.sib = h->d_sib.as<u32>();
    K.slot_tag = h->d_type_tag.as<uint8_t>();
  }
}

// What the plan (plan_host.inc) needs to know about this build.  CNS_SELECT_KERNEL=legacy|pipe|wide... forces a family (A/B
// measurements, and the parity tests run them all); the defaults of a build:
#ifndef CNS_DEFAULT_PIPE
#define CNS_DEFAULT_PIPE 1
#endif
#ifndef CNS_DEFAULT_WIDE
#define CNS_DEFAULT_WIDE 1
#endif
constexpr u32 kGiantHelperBudget = 64;   // helper workgroups of a k_giant launch at most (plan_host.inc: plan_serial_launch)
#define CNS_WIDTH(w) (u32)(w),
constexpr u32 kSelectWidths[] = {CNS_NPL_LIST(CNS_WIDTH)}, kPipeWidths[] = {CNS_PNPL_LIST(CNS_WIDTH)};
#undef CNS_WIDTH
static_assert(CNS_KERNEL_AUTO == cns_plan::kPinAuto && CNS_KERNEL_SELECT == cns_plan::kPinSelect, "plan_host.inc: cns_kernel_pin");
static_assert(kSelectWidths[sizeof kSelectWidths / 4 - 1] == CNS_NPL_MAX && kPipeWidths[sizeof kPipeWidths / 4 - 1] == (u32)kPNplMax, "the lists end in their widest tile");
template <class W>
cns_plan::WideBuild wide_build() {
  cns_plan::WideBuild b;
  b.waves = W::waves; b.group = W::group; b.max_parts = W::max_parts; b.aux_max = W::aux_max; b.last_in_lds_rows = W::last_in_lds_rows;
  b.tiles.lanes = W::lanes; b.tiles.block = W::block;
  b.tiles.widths.assign(std::begin(W::widths), std::end(W::widths));
  b.window_widths.assign(W::widths, W::widths + W::window_widths);
  return b;
}
const cns_plan::Facts& plan_facts() {
  static const cns_plan::Facts F = [] {
    cns_plan::Facts f;
    f.wide[0] = wide_build<w64::WideInfo>(); f.wide[1] = wide_build<w32::WideInfo>(); f.wide[2] = wide_build<w16::WideInfo>(); f.wide[3] = wide_build<w8::WideInfo>();
    f.select.lanes = kScan; f.select.block = kBlock; f.select.widths.assign(std::begin(kSelectWidths), std::end(kSelectWidths));
    f.pipe.lanes = kPScan; f.pipe.block = kPBlock; f.pipe.widths.assign(std::begin(kPipeWidths), std::end(kPipeWidths));
#ifdef CNS_ONLY_NPL   // experiment builds: one tile width only
    f.only_npl = CNS_ONLY_NPL;
#endif
    f.mem_slots = w8::WideInfo::mem_slots; f.giant_mem_slots = w8::WideInfo::giant_mem_slots;
    f.giant_helpers_max = w8::kGiantHelpersMax; f.giant_helper_budget = kGiantHelperBudget;
    f.default_wide = CNS_DEFAULT_WIDE != 0; f.default_pipe = CNS_DEFAULT_PIPE != 0;
    return f;
  }();
  return F;
}
// The shipped build's figures as tests/cpp/plan_host_test.cpp writes them out (experiment builds change them at will).
#if defined(CNS_WIDE_WGS_ALL) && !defined(CNS_ONLY_NPL) && !defined(CNS_WIDE_AUX_CAP) && CNS_BLOCK == 512 && CNS_IDLE_WAVE >= 8 && CNS_PIPE_BLOCK == 768 && CNS_PIPE_TESTERS == 3 && CNS_WIDE_SPW == 4 && CNS_WIDE_WIN == 32
template <class W, u32... Ws>
constexpr bool wide_is(u32 waves, u32 group, u32 max_parts, u32 lanes, u32 aux_max, u32 windows) {
  constexpr u32 ws[] = {Ws...};
  if (sizeof ws != sizeof W::widths) return false;
  for (size_t i = 0; i < sizeof ws / 4; ++i) if (ws[i] != W::widths[i]) return false;
  return W::waves == waves && W::group == group && W::max_parts == max_parts && W::lanes == lanes && W::aux_max == aux_max && W::window_widths == windows &&
         W::last_in_lds_rows == 4 && W::block == 512;
}
static_assert(wide_is<w64::WideInfo, 1, 2, 4, 8, 16>(64, 17, 8, 4096, 3, 2) && wide_is<w32::WideInfo, 1, 2, 4, 8>(32, 9, 24, 2048, 1, 0) &&
              wide_is<w16::WideInfo, 1, 2, 4, 8>(16, 5, 48, 1024, 1, 0) && wide_is<w8::WideInfo, 1, 2, 4, 8>(8, 3, 80, 512, 1, 0), "plan_host_test.cpp: k_wide's builds");
static_assert(kScan == 448 && kBlock == 512 && sizeof kSelectWidths == 24 && kSelectWidths[0] == 1 && kSelectWidths[1] == 3 && kSelectWidths[2] == 10 &&
              kSelectWidths[3] == 19 && kSelectWidths[4] == 28 && kSelectWidths[5] == 37, "plan_host_test.cpp: k_select's tiles");
static_assert(kPScan == 512 && kPBlock == 768 && sizeof kPipeWidths == 16 && kPipeWidths[0] == 1 && kPipeWidths[1] == 4 && kPipeWidths[2] == 8 && kPipeWidths[3] == 16,
              "plan_host_test.cpp: k_pipe's tiles");
static_assert(w8::WideInfo::mem_slots == 143360 && w8::WideInfo::giant_mem_slots == 544768 && w8::kGiantHelpersMax == 64 && kGiantHelperBudget == 64 &&
              CNS_DEFAULT_WIDE == 1 && CNS_DEFAULT_PIPE == 1, "plan_host_test.cpp: k_mem / k_giant, the defaults");
#endif

// One launch of a cycle: its stream, its copy of the parameter block in HBM (the out-of-line routines read that one) and the
// workgroups of the cycle's other launches (they hold CUs while a kernel whose workgroups wait needs all of its own resident).
struct LaunchCtx {
  hipStream_t stream;
  const KParams* dparams;
  u32 other_blocks;
};
enum class Launched { Yes, NotProven, HipError };
struct CtlBuf { DevBuf* buf; size_t bytes; };   // a control buffer to size and zero before the launch (0 bytes: not used)
// One launch of the k_wide family (k_wide, k_mem, k_giant): `edit` points the kernel's parameter block at the zeroed control buffers.
// `whole_block`: the device copy of the block gets all of it (k_mem, k_giant); else only wide_ctl — the caller uploaded the rest (k_wide).
template <class Edit>
Launched launch_wide_family(const void* fn, const cns_plan::Candidate& c, const KParams& K, const LaunchCtx& L, u32 num_cus,
                            std::initializer_list<CtlBuf> ctl, bool whole_block, Edit edit) {
  // A pad of dynamic LDS keeps the kernel at one workgroup per CU (one scanner wave per SIMD is the point of k_wide).
  size_t dyn = 0;
  hipFuncAttributes fa;
  if (hipFuncGetAttributes(&fa, fn) == hipSuccess && fa.sharedSizeBytes < 84u * 1024u) {
    dyn = 84u * 1024u - fa.sharedSizeBytes;
    if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn) != hipSuccess) { dyn = 0; (void)hipGetLastError(); }
  }
  // The workgroups of a candidate that `waits` spin on each other: ALL of them must be resident at once.  Proof, not assumption: the
  // runtime's own occupancy figure for this kernel at this block size and LDS footprint, times the device's CUs, must cover the grid
  // and what the cycle's other launches hold — else the launch is refused here and the caller takes the plan's next candidate
  // (k_pipe / k_select, k_mem), which needs no co-residency.
  if (c.waits) {
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, (int)c.block, dyn) != hipSuccess) { (void)hipGetLastError(); per_cu = 0; }
    if (per_cu < 1 || (u64)per_cu * num_cus < (u64)c.grid + L.other_blocks) return Launched::NotProven;
  }
  for (const CtlBuf& b : ctl)
    if (b.bytes && (b.buf->ensure(b.bytes) != hipSuccess || hipMemsetAsync(b.buf->p, 0, b.bytes, L.stream) != hipSuccess)) return Launched::HipError;
  KParams K2 = K;
  edit(K2);
  KParams* dp = const_cast<KParams*>(L.dparams);
  if ((whole_block ? hipMemcpyAsync(dp, &K2, sizeof(KParams), hipMemcpyHostToDevice, L.stream)
                   : hipMemcpyAsync(&dp->wide_ctl, &K2.wide_ctl, sizeof(char*), hipMemcpyHostToDevice, L.stream)) != hipSuccess) return Launched::HipError;
  const KParams* dparams = L.dparams;
  void* args[2] = {(void*)&K2, (void*)&dparams};
  return hipLaunchKernel(fn, dim3(c.grid), dim3(c.block), args, dyn, L.stream) == hipSuccess ? Launched::Yes : Launched::HipError;
}
// k_wide: 1 + 8 (or 1 + 16, ...) workgroups per partition plus the candidate's extra homes.
template <class W>
Launched launch_wide(cns_engine* h, const KParams& K, const LaunchCtx& L, const cns_plan::Candidate& c) {
  const char* kname = "";
  const void* fn = W::pick(W::lanes * c.width, &kname, c.windows);
  const bool last_in_hbm = c.width > W::last_in_lds_rows;   // 8 / 16 rows per lane: the home workgroup's last-task table does not fit the LDS
  return launch_wide_family(fn, c, K, L, h->num_cus, {{&h->d_wide, (size_t)h->rlay.P * W::ctl_bytes}, {&h->d_wide_last, last_in_hbm ? (size_t)h->rlay.P * W::lanes * W::npl_max * sizeof(u32) : 0}},
                            false, [&](KParams& K2) {
                              K2.wide_ctl = h->d_wide.as<char>();
                              K2.wide_aux = c.extra;
                              if (last_in_hbm) K2.wide_last = h->d_wide_last.as<u32>();
                            });
}
// k_mem — groups of partitions that share nodes and are wider than k_select's register tile (an "ALL" partition over a large cluster):
// k_wide's HOME workgroup alone, every job through the sequential protocol with its tester waves as memory scanners over the
// committed HBM arrays (KParams::serial_only).  The narrowest build serves (its two scanner workgroups per partition leave at once);
// no workgroup waits for another one.  Slow — every job reads every slot of its group — and exact.  Above W::mem_slots (143 360) the
// giant instantiation (19-word row masks, up to W::giant_mem_slots) serves the launch: same protocol, more scratch per memory-scanner
// lane; the launches that fit the ordinary masks keep the ordinary kernel.
// k_giant (wide_kernel.inc, "k_giant"): the giant instantiation in serial-only mode plus the candidate's helper workgroups per partition
// that scan stripes of the job's slots; grid = nparts x (1 + helpers).  The helpers and the home wait for each other.
Launched launch_serial(cns_engine* h, const KParams& K, const LaunchCtx& L, const cns_plan::Candidate& c) {
  using W = w8::WideInfo;
  const bool giant = c.family == cns_plan::Family::Giant;
  const void* fn = c.giant_masks ? (const void*)w8::k_wide<1, false, w8::kWMemWordsGiant> : (const void*)w8::k_wide<1, false>;
  return launch_wide_family(fn, c, K, L, h->num_cus, {{&h->d_wide_mem, (size_t)h->rlay.P * W::ctl_bytes}, {&h->d_giant, giant ? (size_t)h->rlay.P * sizeof(w8::GiantCtl) : 0}},
                            true, [&](KParams& K2) {
                              K2.wide_ctl = h->d_wide_mem.as<char>();
                              K2.serial_only = 1;
                              if (giant) { K2.giant_ctl = h->d_giant.as<char>(); K2.giant_nh = c.extra; }
                            });
}
// One launch of the plan: its candidates in order, the first that launches in *chosen.  0 ok, else a status (h->err is set).
int run_launch(cns_engine* h, const KParams& K, hipStream_t stream, const KParams* dparams, const cns_plan::Launch& PL, cns_plan::Candidate* chosen) {
  using cns_plan::Family;
  const LaunchCtx L{stream, dparams, PL.other_blocks};
  for (const cns_plan::Candidate& c : PL.cands) {
    Launched r = Launched::Yes;
    switch (c.family) {
      case Family::Wide:
        r = c.build == 0 ? launch_wide<w64::WideInfo>(h, K, L, c) : c.build == 1 ? launch_wide<w32::WideInfo>(h, K, L, c)
          : c.build == 2 ? launch_wide<w16::WideInfo>(h, K, L, c) : launch_wide<w8::WideInfo>(h, K, L, c);
        break;
      case Family::Mem: case Family::Giant: r = launch_serial(h, K, L, c); break;
      case Family::Pipe:
#define CNS_LAUNCH_WIDTH(w) if (c.width == (w)) hipLaunchKernelGGL((k_pipe<w>), dim3(c.grid), dim3(c.block), 0, L.stream, K, L.dparams);
        CNS_PNPL_LIST(CNS_LAUNCH_WIDTH)
#undef CNS_LAUNCH_WIDTH
        break;
      case Family::Select:
#ifdef CNS_ONLY_NPL
        hipLaunchKernelGGL((k_select<CNS_ONLY_NPL>), dim3(c.grid), dim3(c.block), 0, L.stream, K, L.dparams);
#else
#define CNS_LAUNCH_WIDTH(w) if (c.width == (w)) hipLaunchKernelGGL((k_select<w>), dim3(c.grid), dim3(c.block), 0, L.stream, K, L.dparams);
        CNS_NPL_LIST(CNS_LAUNCH_WIDTH)
#undef CNS_LAUNCH_WIDTH
#endif
        break;
    }
    if (r == Launched::HipError) return fail(h, CNS_ERR_HIP, c.family == Family::Wide ? "k_wide: control block allocation / upload / launch failed"
                                                                                     : "k_mem / k_giant: control block allocation / upload / launch failed");
    if (r == Launched::Yes) { *chosen = c; return 0; }
  }
  return fail(h, CNS_ERR_UNSUPPORTED, PL.exhausted);
}

// v on the device; an empty vector as one zero element (a kernel's table pointer always names something)
template <class T>
int upload_some(cns_engine* h, DevBuf& b, const std::vector<T>& v) {
  static const T zero{};
  return v.empty() ? stage(h, b, &zero, sizeof(T)) : upload(h, b, v);
}

int upload_running(cns_engine* h) {
  if (int rc = upload(h, h->d_rn_off, h->run.rn_off)) return rc;
  if (int rc = upload_some(h, h->d_rn_end, h->run.rn_end)) return rc;
  if (int rc = upload_some(h, h->d_rn_res, h->run.rn_res)) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return 0;
}

// The handle's layout (h->lay, h->rlay: snapshot_host.inc) on the device and the per-slot buffers sized for it.  Running jobs must be
// set again after the layout changed: none until cns_set_running, on the host as on the device.
int upload_snapshot(cns_engine* h) {
  const cns_snapshot::ResvLayout& X = h->rlay;
  (void)cns_snapshot::build_running(h->lay, X, nullptr, h->run);
  ++h->lay_gen; h->rl_dev = false; h->rp_index = h->rp_call = false;   // (a ledger survives; its per-slot tables come back with the next cns_running_advance)
  if (h->lay.shared) {
    if (int rc = upload(h, h->d_slot_block, X.slot_block)) return rc;
    if (int rc = upload(h, h->d_sib_off, X.sib_off)) return rc;
    if (int rc = upload_some(h, h->d_sib, X.sib)) return rc;
    if (int rc = upload(h, h->d_type_tag, X.slot_tag)) return rc;   // per slot: member partition inside the group
    if (int rc = upload(h, h->d_tag_base, X.tag_base)) return rc;
    if (int rc = upload(h, h->d_tag_off, X.tag_off)) return rc;
  }
  std::vector<i64> resv_se;
  for (u32 v = 0; v < X.V; ++v) { resv_se.push_back(X.resv_start[v]); resv_se.push_back(X.resv_end[v]); }
  if (int rc = upload(h, h->d_part_off, X.part_off)) return rc;
  if (int rc = upload(h, h->d_slot_node, X.slot_node)) return rc;
  if (int rc = upload(h, h->d_slot_total, X.slot_total)) return rc;
  if (int rc = upload(h, h->d_slot_end, X.slot_end)) return rc;
  if (int rc = upload_some(h, h->d_slot_type, X.slot_type)) return rc;
  if (int rc = upload(h, h->d_type_total, X.type_total)) return rc;
  if (int rc = upload(h, h->d_rv_off, X.rv_off)) return rc;
  if (int rc = upload_some(h, h->d_rv_start, X.rv_start)) return rc;
  if (int rc = upload_some(h, h->d_rv_end, X.rv_endt)) return rc;
  if (int rc = upload_some(h, h->d_rv_res, X.rv_res)) return rc;
  if (int rc = upload_some(h, h->d_resv_se, resv_se)) return rc;
  const size_t S1 = std::max<u32>(X.S, 1);
  const std::pair<DevBuf*, size_t> per_slot[] = {   // (d_blocks: 64.6 KB per node — HBM is plentiful; d_flen: groups only)
      {&h->d_blocks, kBlockStride}, {&h->d_cost, sizeof(double)}, {&h->d_fcpu, sizeof(int)}, {&h->d_fmem, sizeof(u32)}, {&h->d_fcnt, sizeof(u64)},
      {&h->d_dipt, sizeof(u32)}, {&h->d_dipcm, sizeof(u32)}, {&h->d_dipg, sizeof(u32)}, {&h->d_first_resv, sizeof(i64)}, {&h->d_bfj, sizeof(u32)},
      {&h->d_gupd, sizeof(UpdRec)}, {&h->d_flen, h->lay.shared ? sizeof(u32) : 0}};
  for (const auto& [buf, elem] : per_slot)
    if (elem) HIPCHK(h, buf->ensure(S1 * elem));
  HIPCHK(h, h->d_heap.ensure((size_t)(X.S + X.P + 1) * sizeof(HeapEnt)));
  HIPCHK(h, h->d_fault.ensure(4 * sizeof(u32)));
  HIPCHK(h, h->d_prof.ensure(((size_t)(X.P + 8) * (size_t)w64::WideInfo::group * 32 + (size_t)X.P * 8 + 2048) * sizeof(u64)));   // (k_wide: blocks > partitions)
  return upload_running(h);   // (its synchronize: resv_se is a local vector)
}

}  // namespace

extern "C" {

int cns_abi_version(void) { return (int)CNS_ABI_VERSION; }

const char* cns_last_error(const cns_handle* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int cns_create(const cns_config* cfg, cns_handle** out) {
  if (!cfg || !out) return fail(nullptr, CNS_ERR_INVALID_ARG, "cns_create: null argument");
  if (cfg->abi_version != CNS_ABI_VERSION) return fail(nullptr, CNS_ERR_INVALID_ARG, "cns_create: ABI version mismatch");
  if (cfg->kernel_pin > CNS_KERNEL_PIPE) return fail(nullptr, CNS_ERR_INVALID_ARG, "cns_create: kernel_pin is not a cns_kernel_pin (a field the caller never zeroed?)");
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev <= 0)
    return fail(nullptr, CNS_ERR_NO_DEVICE, std::string("no HIP device: ") + hipGetErrorString(e) +
                                                " (the engine has no CPU fallback)");
  if (cfg->device < 0 || cfg->device >= ndev) return fail(nullptr, CNS_ERR_INVALID_ARG, "cns_create: bad device ordinal");
  cns_engine* h = new (std::nothrow) cns_engine();
  if (!h) return fail(nullptr, CNS_ERR_HIP, "out of host memory");
  h->cfg = *cfg;
  if (h->cfg.max_job_num_per_node == 0) h->cfg.max_job_num_per_node = 1000;  // kAlgoMaxJobNumPerNode
  if (h->cfg.max_time_window_sec == 0) h->cfg.max_time_window_sec = 7 * 24 * 3600;  // kAlgoMaxTimeWindow
  if (h->cfg.max_job_num_per_node + 2 > kTlCap) {
    delete h;
    return fail(nullptr, CNS_ERR_UNSUPPORTED, "max_job_num_per_node > 1006");
  }
  h->device = cfg->device;
  if ((e = hipSetDevice(h->device)) != hipSuccess || (e = hipStreamCreate(&h->stream)) != hipSuccess) {
    std::string m = hipGetErrorString(e);
    delete h;
    return fail(nullptr, CNS_ERR_HIP, "device/stream init: " + m);
  }
  {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->device) == hipSuccess && cus > 0) h->num_cus = (u32)cus;
    else (void)hipGetLastError();
  }
  for (auto& ev : h->ev)
    if ((e = hipEventCreate(&ev)) != hipSuccess) {
      std::string m = hipGetErrorString(e);
      cns_destroy(h);
      return fail(nullptr, CNS_ERR_HIP, "hipEventCreate: " + m);
    }
  if ((e = hipStreamCreate(&h->stream2)) != hipSuccess || (e = hipEventCreateWithFlags(&h->ev2[0], hipEventDisableTiming)) != hipSuccess ||
      (e = hipEventCreateWithFlags(&h->ev2[1], hipEventDisableTiming)) != hipSuccess) {
    std::string m = hipGetErrorString(e);
    cns_destroy(h);
    return fail(nullptr, CNS_ERR_HIP, "second stream: " + m);
  }
  *out = h;
  return CNS_OK;
}

void cns_destroy(cns_handle* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  for (void* p : h->host_bufs) (void)hipHostFree(p);   // cns_host_alloc
  h->host_bufs.clear();
  if (h->comm) (void)ncclCommDestroy((ncclComm_t)h->comm);
  for (auto& ev : h->ev) if (ev) (void)hipEventDestroy(ev);
  for (auto& ev : h->ev2) if (ev) (void)hipEventDestroy(ev);
  if (h->stream2) (void)hipStreamDestroy(h->stream2);
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;   // every DevBuf and PinBuf releases itself
}

static void valid_keep_nodes(cns_handle* h, const cns_node_soa* nd);   // valid_host.inc
// The three calls of the snapshot: argument and state checks here, the layout in snapshot_host.inc (built into a local: a call that
// fails validation leaves the handle's snapshot, host mirror and device buffers, as it was), then the uploads.
int cns_set_nodes(cns_handle* h, const cns_node_soa* nd) {
  if (!h || !nd) return fail(h, CNS_ERR_INVALID_ARG, "cns_set_nodes: null argument");
  h->refused_probe.clear();
  if (!nd->cpu_total_raw || !nd->mem_total || !nd->core_lo || !nd->part_offsets || (!nd->part_nodes && nd->part_offsets[nd->num_partitions]))
    return fail(h, CNS_ERR_INVALID_ARG, "cns_set_nodes: missing array");
  if (nd->num_nodes == 0 || nd->num_partitions == 0) return fail(h, CNS_ERR_INVALID_ARG, "cns_set_nodes: empty cluster");
  HIPCHK(h, hipSetDevice(h->device));
  if (int rc = build_gres(h, nd->gres)) return rc;
  h->have_nodes = h->have_jobs = h->have_run = false;
  h->rq_have = false;   // (the per-node tables of cns_resvq_set_state index the nodes of the snapshot they were built for)
  u64 all_gres = 0;
  for (u32 c = 0; c < h->gres.num_classes; ++c) all_gres |= h->gres.class_mask[c];
  cns_snapshot::Layout lay;
  cns_snapshot::ResvLayout rlay;
  cns_snapshot::Status st = cns_snapshot::build_layout(nd, all_gres, kCaps, lay, &h->refused_probe);
  if (!st) st = cns_snapshot::build_resv(lay, nullptr, rlay);
  if (st) return fail(h, st.code, st.msg);
  h->lay = std::move(lay); h->rlay = std::move(rlay);
  if (int rc = upload_snapshot(h)) return rc;
  valid_keep_nodes(h, nd);   // (cns_validate_jobs derives its tables from these at its first call)
  h->have_nodes = true;
  return CNS_OK;
}

int cns_set_reservations(cns_handle* h, const cns_resv_soa* rv) {
  if (!h) return fail(h, CNS_ERR_INVALID_ARG, "cns_set_reservations: null handle");
  if (!h->have_nodes) return fail(h, CNS_ERR_STATE, "cns_set_reservations before cns_set_nodes");
  HIPCHK(h, hipSetDevice(h->device));
  h->have_jobs = h->have_run = false;
  cns_snapshot::ResvLayout rlay;
  if (const cns_snapshot::Status st = cns_snapshot::build_resv(h->lay, rv, rlay)) return fail(h, st.code, st.msg);
  h->rlay = std::move(rlay);
  h->vd_rv_have = false;   // (cns_validate_jobs rebuilds its table of the reservations' nodes)
  return upload_snapshot(h);
}

int cns_set_running(cns_handle* h, const cns_running_soa* rn) {
  if (!h) return fail(h, CNS_ERR_INVALID_ARG, "cns_set_running: null handle");
  if (!h->have_nodes) return fail(h, CNS_ERR_STATE, "cns_set_running before cns_set_nodes");
  HIPCHK(h, hipSetDevice(h->device));
  cns_snapshot::RunLayout run;
  if (const cns_snapshot::Status st = cns_snapshot::build_running(h->lay, h->rlay, rn, run)) return fail(h, st.code, st.msg);
  h->run = std::move(run);
  h->rl_have = h->rl_dev = false; h->rp_index = h->rp_call = false;   // (the ledger of cns_running_seed describes another set now)
  h->ra_have = h->ra_sums = false;
  if (int rc = upload_running(h)) return rc;
  h->have_run = false;
  return CNS_OK;
}

static int upload_jobs_impl(cns_handle* h, const cns_job_soa* jb);
// The caller owns its arrays again when the call is back — on EVERY path: an error behind the first asynchronous copy (a failed allocation, a
// queue that fails validation) returns only after the copies from the caller's arrays have drained.
int cns_upload_jobs(cns_handle* h, const cns_job_soa* jb) {
  const int rc = upload_jobs_impl(h, jb);
  if (rc != 0 && h && h->have_nodes) drain(h);
  return rc;
}
static int upload_jobs_impl(cns_handle* h, const cns_job_soa* jb) {
  if (!h || !jb) return fail(h, CNS_ERR_INVALID_ARG, "cns_upload_jobs: null argument");
  if (!h->have_nodes) return fail(h, CNS_ERR_STATE, "cns_upload_jobs before cns_set_nodes");
  if (int rc = table_check(h, jb, kQueueMsgs)) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  hipEvent_t e0 = h->ev[0], e1 = h->ev[1];
  HIPCHK(h, hipEventRecord(e0, h->stream));
  h->have_jobs = h->have_run = false;
  JobTable& T = h->q;
  const u64 batch = h->cfg.scheduled_batch_size ? std::min<u64>(h->cfg.scheduled_batch_size, jb->num_jobs) : jb->num_jobs;
  // The copies of the caller's arrays first: both host passes run in their shadow.  A queue that fails validation returns only after
  // they have drained (cns_upload_jobs).  Offsets without their node list are reported behind the checks of pass 1, which come first.
  if (int rc = table_stage(h, T, jb)) return rc;
  // BasicPriority (JobScheduler.h:185-200) + the per-job pre-checks of the ordered loop (cpp:6744-6761)
  cns_jobs_host::Out O;
  if (int rc = table_route(h, T, jb, batch, "", O)) return rc;
  if (int rc = table_lists_check(h, jb, kQueueMsgs)) return rc;
  h->part_jobs.resize(h->rlay.P);
  for (u32 p = 0; p < h->rlay.P; ++p) h->part_jobs[p] = O.pj_off[p + 1] - O.pj_off[p];
  if (int rc = table_layout(h, T, jb, O)) return rc;
  if (int rc = table_pack(h, T, jb)) return rc;
  if (int rc = upload(h, h->d_pj_off, O.pj_off)) return rc;
  HIPCHK(h, hipEventRecord(e1, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  float ms = 0;
  HIPCHK(h, hipEventElapsedTime(&ms, e0, e1));
  h->timing = cns_timing{};
  h->timing.h2d_ms = ms;
  h->jobs_ordered = batch; h->algo_bytes = O.algo; h->window_shaped = O.n_shaped;
  h->have_jobs = true;
  return CNS_OK;
}

// One pass of the cycle on the device.  *fault_code: the device fault it ended with (0: none).
// `protocol_off`: the retry — no kernel whose workgroups wait for each other.
static int run_resident_once(cns_handle* h, int64_t now, const RunKnobs& kn, bool protocol_off, u32* fault_code) {
  *fault_code = 0;
  h->pass_waits = false;
  h->have_probes = h->probes_answered = false;   // (probes are routed against the snapshot of the cycle they follow)
  HIPCHK(h, hipSetDevice(h->device));
  KParams K;
  fill_params(h, K, now, kn);
  HIPCHK(h, hipEventRecord(h->ev[0], h->stream));
  if (int rc = table_reset(h, h->q)) return rc;
  HIPCHK(h, hipMemsetAsync(h->d_fault.p, 0, 16, h->stream));
  if (h->pre_active) {
    // The mutable preemption state starts every PASS empty, not every call: the retry after a k_wide protocol fault re-runs the
    // k_select partitions too, and a second pass over a first pass's per-slot job lists (slot_head / rec_next), hidden
    // candidates (ent_gone / rec_gone) and preempted pairs (out_cnt) would loop on a self-linked list or report pairs twice.
    DevBuf* B = h->d_pre;
    const cns_preempt::Plan& L = h->pre_plan;
    HIPCHK(h, hipMemsetAsync(B[B_ENTGONE].p, 0, L.ent_gone, h->stream));
    HIPCHK(h, hipMemsetAsync(B[B_HEAD].p, 0xFF, L.slot_head, h->stream));
    HIPCHK(h, hipMemsetAsync(B[B_RECGONE].p, 0, L.rec_gone, h->stream));
    HIPCHK(h, hipMemsetAsync(h->pre_params.out_cnt, 0, L.cnt_bytes, h->stream));
  }
  HIPCHK(h, hipMemsetAsync(h->d_prof.p, 0, ((size_t)h->rlay.P * (32 + 16) + 2048) * sizeof(u64), h->stream));   // cycle counters + the always-on protocol counters
  HIPCHK(h, h->d_params.ensure(sizeof(KParams)));
  HIPCHK(h, hipMemcpyAsync(h->d_params.p, &K, sizeof(KParams), hipMemcpyHostToDevice, h->stream));
  if (h->rlay.S) hipLaunchKernelGGL(k_init_nodes, dim3((h->rlay.S + 255) / 256), dim3(256), 0, h->stream, h->d_params.as<KParams>());
  if (h->q.Jg) hipLaunchKernelGGL(k_prep_jobs, dim3((unsigned)((h->q.Jg + 255) / 256)), dim3(256), 0, h->stream, h->d_params.as<KParams>(), (u64)h->q.Jg);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipEventRecord(h->ev[1], h->stream));
  bool split = false;
  cns_plan::Candidate ca, cb, cc;   // what launched for the plan's a / b / c
  if (h->q.Jg) {
    cns_plan::Inputs in;
    in.parts.resize(h->rlay.P);
    for (u32 p = 0; p < h->rlay.P; ++p)
      in.parts[p] = {p < h->part_jobs.size() ? h->part_jobs[p] : 0, h->rlay.part_off[p + 1] - h->rlay.part_off[p], p < h->lay.eng_members.size() ? h->lay.eng_members[p] : 1u,
                     p < h->pre_part.size() && h->pre_part[p]};
    in.pre_active = h->pre_active; in.num_cus = h->num_cus; in.kernel_pin = h->cfg.kernel_pin;
    in.sw = kn.sw; in.protocol_off = protocol_off; in.wide_window = K.wide_window; in.aux_override = kn.aux;
    cns_plan::CyclePlan plan = cns_plan::plan_cycle(plan_facts(), in);
    if (plan.unsupported) return fail(h, CNS_ERR_UNSUPPORTED, plan.error);
    const bool has_c = !plan.c.parts.empty();
    if (has_c) {
      if (int rc = upload(h, h->d_pmap_c, plan.c.parts)) return rc;
      HIPCHK(h, h->d_params3.ensure(sizeof(KParams)));
      KParams KC = K;
      KC.part_map = h->d_pmap_c.as<u32>(); KC.launch_parts = (u32)plan.c.parts.size();
      KC.general_only = 0; KC.pre = PreParams{};
      HIPCHK(h, hipEventRecord(h->ev2[0], h->stream));                  // tables + init kernels done: the second stream may start
      HIPCHK(h, hipStreamWaitEvent(h->stream2, h->ev2[0], 0));
      if (int rc = run_launch(h, KC, h->stream2, h->d_params3.as<KParams>(), plan.c, &cc)) return rc;
      // (the other launches were planned beside c's first candidate: where k_giant's helpers were not proven, beside k_mem's home workgroups instead)
      if (cc.family != plan.c.cands[0].family) { in.helpers_unproven = true; plan = cns_plan::plan_cycle(plan_facts(), in); }
    }
    if (const cns_plan::Launch* one = plan.single()) {
      // one launch: over all partitions (identity map) when every one is busy, else over the busy ones (part_map)
      const bool plain = one == &plan.a;
      KParams K1 = K;
      if (plain) { K1.general_only = 0; K1.pre = PreParams{}; }
      if (!plan.identity) {
        if (int rc = upload(h, h->d_pmap_a, one->parts)) return rc;
        K1.part_map = h->d_pmap_a.as<u32>(); K1.launch_parts = (u32)one->parts.size();
      }
      if (K1.general_only != K.general_only || !plan.identity) HIPCHK(h, hipMemcpyAsync(h->d_params.p, &K1, sizeof(KParams), hipMemcpyHostToDevice, h->stream));
      if (int rc = run_launch(h, K1, h->stream, h->d_params.as<KParams>(), *one, plain ? &ca : &cb)) return rc;
    } else if (plan.split) {
      if (int rc = upload(h, h->d_pmap_a, plan.a.parts)) return rc;
      if (int rc = upload(h, h->d_pmap_b, plan.b.parts)) return rc;
      HIPCHK(h, h->d_params2.ensure(sizeof(KParams)));
      KParams KA = K, KB = K;
      KA.part_map = h->d_pmap_a.as<u32>(); KA.launch_parts = (u32)plan.a.parts.size();
      KA.general_only = 0; KA.pre = PreParams{};
      KA.slot_block = nullptr; KA.sib_off = nullptr; KA.sib = nullptr; KA.slot_tag = nullptr;   // (none of these partitions shares a node)
      KB.part_map = h->d_pmap_b.as<u32>(); KB.launch_parts = (u32)plan.b.parts.size();
      HIPCHK(h, hipMemcpyAsync(h->d_params.p, &KA, sizeof(KParams), hipMemcpyHostToDevice, h->stream));
      HIPCHK(h, hipMemcpyAsync(h->d_params2.p, &KB, sizeof(KParams), hipMemcpyHostToDevice, h->stream));
      HIPCHK(h, hipEventRecord(h->ev2[0], h->stream));                  // tables + init kernels done: the second stream may start
      HIPCHK(h, hipStreamWaitEvent(h->stream2, h->ev2[0], 0));
      if (int rc = run_launch(h, KB, h->stream2, h->d_params2.as<KParams>(), plan.b, &cb)) return rc;   // first: its few workgroups take their CUs
      if (int rc = run_launch(h, KA, h->stream, h->d_params.as<KParams>(), plan.a, &ca)) return rc;
      HIPCHK(h, hipEventRecord(h->ev[3], h->stream));                   // the partitions on the fast kernels are done here
      split = true;
    }
    if (has_c || split) {   // the cycle ends when the launch(es) on the second stream have
      HIPCHK(h, hipEventRecord(h->ev2[1], h->stream2));
      HIPCHK(h, hipStreamWaitEvent(h->stream, h->ev2[1], 0));
    }
    h->last_kernel = cns_plan::last_kernel_text(plan, plan.a.parts.empty() ? nullptr : &ca, plan.b.parts.empty() ? nullptr : &cb, has_c ? &cc : nullptr);
    // (k_wide serves plain launches only — a, the launch last_kernel names first — and k_giant only c: b's k_select never waits)
    h->pass_waits = (!plan.a.parts.empty() && ca.waits) || (has_c && cc.waits);
    HIPCHK(h, hipGetLastError());
  }
  HIPCHK(h, hipEventRecord(h->ev[2], h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  float a = 0, b = 0;
  HIPCHK(h, hipEventElapsedTime(&a, h->ev[0], h->ev[1]));
  HIPCHK(h, hipEventElapsedTime(&b, h->ev[1], h->ev[2]));
  h->timing.init_ms = a;
  h->timing.select_ms = b;
  if (split) {   // a split cycle: when the partitions on the fast kernels were done (the cycle itself ends with the slower launch)
    float c = 0;
    HIPCHK(h, hipEventElapsedTime(&c, h->ev[1], h->ev[3]));
    char buf[64];
    snprintf(buf, sizeof buf, " [%s partitions done after %.1f ms]", cns_plan::kernel_of(ca).c_str(), c);
    h->last_kernel += buf;
  }
  h->timing.jobs_ordered = h->jobs_ordered;
  h->timing.algorithmic_bytes = h->algo_bytes;
  u32 fault[4] = {0, 0, 0, 0};
  HIPCHK(h, hipMemcpy(fault, h->d_fault.p, 16, hipMemcpyDeviceToHost));
  h->last_now = now;
  if (fault[0] && h->pre_active && (fault[0] == 31 || fault[0] == 32)) {
    *fault_code = fault[0];
    return fail(h, CNS_ERR_UNSUPPORTED, std::string("cns_select_preempt: job ") + std::to_string(fault[1]) + (fault[0] == 31
                    ? " has more preemption candidates on its nodes than the candidate buffer holds"
                    : " needs more segment-tree nodes than the per-partition pool (" + std::to_string(kPrePoolNodes) + ") holds") +
                    "; keep the CPU SchedulerAlgo for this cycle (include/crane_gpu/preempt.h, limits)");
  }
  if (fault[0]) {
    *fault_code = fault[0];
    return fail(h, CNS_ERR_DEVICE_FAULT, "device invariant violated: code " + std::to_string(fault[0]) + " job " +
                                             std::to_string(fault[1]) + " aux " + std::to_string(fault[2]) + "," +
                                             std::to_string(fault[3]) + " (" + h->last_kernel + ")");
  }
  h->have_run = true;
  h->run_preempt = h->pre_call;
  h->run_preempt_rl = false;   // (cns_running_select_preempt sets it behind its cycle)
  return CNS_OK;
}

// k_wide is a persistent kernel whose workgroups wait for each other; its waits are bounded and end in a device fault
// (codes 20..41: a wait of the exchange / command / task-ring protocol ran out, or a protocol position did not match).
// Such a fault says nothing about the INPUT: the cycle is re-run once on k_pipe / k_select, which live inside one
// workgroup per partition (every run starts from the caller's tables: k_init_nodes, k_prep_jobs and the result buffers
// are part of the pass).  Faults below 20 are data invariants of the shared routines (e.g. 3: the input class on which
// the reference itself asserts) and would recur: they fail the call.
int cns_run_resident(cns_handle* h, int64_t now) {
  if (!h) return fail(h, CNS_ERR_INVALID_ARG, "cns_run_resident: null handle");
  if (!h->have_nodes || !h->have_jobs) return fail(h, CNS_ERR_STATE, "cns_run_resident before set_nodes/upload_jobs");
  u32 code = 0;
  const RunKnobs kn = RunKnobs::read();
  int rc = run_resident_once(h, now, kn, false, &code);
  // (CNS_WIDE_NO_RETRY=1: the fault fails the call — the GPU parity tests run that way, so that a k_wide that breaks is seen
  // and not papered over by the kernels behind it)
  // (k_giant's helpers wait for the home and the home for them: a fault of that protocol, 43, is re-run the same way, on k_mem)
  if (rc == CNS_ERR_DEVICE_FAULT && code >= 20 && h->pass_waits && !kn.no_retry) {
    const std::string first = h->err;
    ++h->wide_retries;
    rc = run_resident_once(h, now, kn, true, &code);
    if (rc == CNS_OK) h->last_kernel += " (retry after: " + first + ")";
    else h->err = first + "; retry on " + h->last_kernel + ": " + h->err;
  }
  return rc;
}

int cns_download(cns_handle* h, cns_placement_soa* out) {
  if (!h || !out) return fail(h, CNS_ERR_INVALID_ARG, "cns_download: null argument");
  if (!h->have_run) return fail(h, CNS_ERR_STATE, "cns_download before a successful run");
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipEventRecord(h->ev[0], h->stream));
  if (int rc = table_download(h, h->q, out, kQueueMsgs)) return rc;
  HIPCHK(h, hipEventRecord(h->ev[1], h->stream));
  table_offsets(h->q, out);
  HIPCHK(h, hipStreamSynchronize(h->stream));
  float ms = 0;
  HIPCHK(h, hipEventElapsedTime(&ms, h->ev[0], h->ev[1]));
  h->timing.d2h_ms = ms;
  return CNS_OK;
}

int cns_host_alloc(cns_handle* h, uint64_t bytes, void** out) {
  if (!h || !out) return fail(h, CNS_ERR_INVALID_ARG, "cns_host_alloc: null argument");
  *out = nullptr;
  HIPCHK(h, hipSetDevice(h->device));
  void* p = nullptr;
  HIPCHK(h, hipHostMalloc(&p, (size_t)std::max<uint64_t>(bytes, 1), hipHostMallocDefault));
  h->host_bufs.insert(p);
  *out = p;
  return CNS_OK;
}

int cns_host_free(cns_handle* h, void* p) {
  if (!h) return fail(h, CNS_ERR_INVALID_ARG, "cns_host_free: null handle");
  if (!p) return CNS_OK;
  auto it = h->host_bufs.find(p);
  if (it == h->host_bufs.end()) return fail(h, CNS_ERR_INVALID_ARG, "cns_host_free: not a buffer of cns_host_alloc on this handle");
  h->host_bufs.erase(it);
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipHostFree(p));
  return CNS_OK;
}

int cns_set_host_threads(cns_handle* h, uint32_t n) {
  if (!h) return fail(h, CNS_ERR_INVALID_ARG, "cns_set_host_threads: null handle");
  if (n > 64) return fail(h, CNS_ERR_INVALID_ARG, "cns_set_host_threads: more than 64 threads");
  h->host_threads = n;
  return CNS_OK;
}

int cns_select(cns_handle* h, int64_t now, const cns_job_soa* jobs, cns_placement_soa* out) {
  if (int rc = cns_upload_jobs(h, jobs)) return rc;
  if (int rc = cns_run_resident(h, now)) return rc;
  return cns_download(h, out);
}

// The cycle of cns_select_preempt / cns_running_select_preempt behind their setup of the running side: the queue is uploaded, the
// end times of the preempting rows are bound.  R running jobs, A entries of the per-slot tables, set_in: the ids of the preempting set
// that still run.  bind_running puts the running side's tables on the device and names them in the parameter block.
// row_ids: the job ids of the preempted running jobs when the caller handed no rn_job_id in (cns_running_select_preempt_attrs).
using PreRowIds = std::function<int(const std::vector<u32>& rows, std::vector<u32>& ids)>;
static int pre_cycle(cns_handle* h, int64_t now, const cns_job_soa* jobs, const cns_preempt_soa* pre, cns_placement_soa* out, cns_preempt_out* pout,
                     const u32 R, const u32 A, const std::vector<u32>& set_in, const std::string& who, const std::function<int(PreParams&)>& bind_running,
                     const PreRowIds* row_ids = nullptr) {
  const u64 J = jobs->num_jobs;
  const auto setup_done = [h] { h->rp_timing.setup_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - h->pre_t0).count(); };
  if (!cns_preempt::any_may_preempt(pre, J)) {
    setup_done();
    if (int rc = cns_run_resident(h, now)) return rc;
    if (int rc = cns_download(h, out)) return rc;
    const auto v = cns_preempt::plain_ending(who, J, set_in, pout);
    return v ? fail(h, v.code, v.msg) : CNS_OK;
  }
  // qos preempt lists, pending-job fields (by queue index)
  const cns_preempt::QosLists ql = cns_preempt::qos_lists(pre);
  cns_preempt::PlanIn in;
  in.J = J; in.places = h->q.places; in.R = R; in.A = A; in.P = h->rlay.P; in.S = h->rlay.S; in.pool_nodes = kPrePoolNodes; in.node_bytes = sizeof(PreNode);
  const cns_preempt::Plan L = h->pre_plan = cns_preempt::plan_buffers(in);
  DevBuf* B = h->d_pre;
  if (int rc = upload(h, B[B_QPOFF], ql.off)) return rc;
  if (int rc = upload(h, B[B_QP], ql.flat)) return rc;
  const std::vector<u32> pj_qos = cns_preempt::padded<u32>(pre->pd_qos, J), pj_qprio = cns_preempt::padded<u32>(pre->pd_qos_priority, J);
  const std::vector<double> pj_prio = cns_preempt::padded<double>(pre->pd_priority, J);
  if (int rc = upload(h, B[B_PJQOS], pj_qos)) return rc;
  if (int rc = upload(h, B[B_PJQP], pj_qprio)) return rc;
  if (int rc = upload(h, B[B_PJPRIO], pj_prio)) return rc;
  HIPCHK(h, B[B_PJREC0].ensure(L.pj4)); HIPCHK(h, B[B_PJK].ensure(L.pj4)); HIPCHK(h, B[B_PJEND].ensure(L.pj8));
  HIPCHK(h, B[B_ENTGONE].ensure(L.ent_gone));   // (zeroed at the start of every pass: run_resident_once)
  HIPCHK(h, B[B_HEAD].ensure(L.slot_head));
  HIPCHK(h, B[B_RECNEXT].ensure(L.rec4)); HIPCHK(h, B[B_RECORIG].ensure(L.rec4)); HIPCHK(h, B[B_RECSLOT].ensure(L.rec4));
  HIPCHK(h, B[B_RECGONE].ensure(L.rec_gone));
  HIPCHK(h, B[B_MISC].ensure(L.misc));   // segment-tree pools | candidate lists | chosen lists | output counter | output pairs
  char* misc = B[B_MISC].as<char>();
  PreParams& Q = h->pre_params;
  Q = PreParams{};
  Q.enabled = 1; Q.num_qos = pre->num_qos;
  Q.qp_off = B[B_QPOFF].as<u32>(); Q.qp = B[B_QP].as<u32>();
  Q.pj_qos = B[B_PJQOS].as<u32>(); Q.pj_qprio = B[B_PJQP].as<u32>(); Q.pj_prio = B[B_PJPRIO].as<double>();
  Q.pj_rec0 = B[B_PJREC0].as<u32>(); Q.pj_k = B[B_PJK].as<u32>(); Q.pj_end = B[B_PJEND].as<i64>();
  Q.ent_gone = B[B_ENTGONE].as<uint8_t>();
  if (int rc = bind_running(Q)) return rc;   // the running side: entry -> job and slot, per job its fields, end, mark and entries
  Q.slot_head = B[B_HEAD].as<u32>(); Q.rec_next = B[B_RECNEXT].as<u32>(); Q.rec_orig = B[B_RECORIG].as<u32>();
  Q.rec_slot = B[B_RECSLOT].as<u32>(); Q.rec_gone = B[B_RECGONE].as<uint8_t>();
  Q.pool = misc; Q.pool_nodes = L.pool_nodes; Q.cand_cap = L.cand_cap;
  Q.cand = (u32*)(misc + L.off_cand); Q.chosen = (u32*)(misc + L.off_chosen);
  Q.out_cnt = (u32*)(misc + L.off_cnt); Q.out = (u32*)(misc + L.off_out); Q.out_cap = L.out_cap;
  // CNS_PREEMPT_TREE=literal: TryPreempt_ on the node-for-node trees only (else: the fall-back of a call that runs out of compressed records)
  { const char* tr = getenv("CNS_PREEMPT_TREE"); Q.literal_tree = (tr && !strcmp(tr, "literal")) ? 1u : ((tr && !strcmp(tr, "tiny")) ? 2u : 0u); }   // tiny: a handful of compressed records per call, the rest falls back
  h->pre_part = cns_preempt::parts_that_may_preempt(pre, J, h->q.job_part, h->rlay.P);   // only they run on k_select's general path (run_resident_once)
  h->pre_active = true;
  setup_done();
  int rc = cns_run_resident(h, now);
  h->pre_active = false;
  if (rc) return rc;
  if (int rc3 = cns_download(h, out)) return rc3;
  // ---- the preempted lists: one copy of the count, one of that many (pending job, reference) pairs; the fold is preempt_host.inc's ----
  u32 cnt = 0;
  HIPCHK(h, hipMemcpy(&cnt, misc + L.off_cnt, 4, hipMemcpyDeviceToHost));
  const u32 held = cnt > L.out_cap ? 0u : cnt;   // (a count past the buffer: the fold refuses before it reads a pair)
  std::vector<u32> pairs((size_t)held * 2 + 2);
  if (held) HIPCHK(h, hipMemcpy(pairs.data(), misc + L.off_out, (size_t)held * 8, hipMemcpyDeviceToHost));
  const cns_preempt::RowIds ids_of = [&](const std::vector<u32>& rows, std::vector<u32>& ids) {
    const int rc4 = (*row_ids)(rows, ids);
    return rc4 ? cns_preempt::refuse(rc4, h->err) : cns_preempt::Verdict{};
  };
  const auto v = cns_preempt::fold(who, cnt, L.out_cap, pairs.data(), J, pre, set_in, row_ids ? &ids_of : nullptr, pout);
  return v ? fail(h, v.code, v.msg) : CNS_OK;
}

// include/crane_gpu/preempt.h.  TryPreempt_ (JobScheduler.cpp:6378-6505) releases resources inside a cycle, which the
// pipelined kernels exclude by construction (node state monotone within a cycle: caches, predicted tiles, decoupled
// commits).  A cycle with preemption enabled therefore runs k_select with every job on its general path
// (KParams::general_only) and the device form of TryPreempt_ / PreemptSegTree between the res_total selection and the
// backfill (csrc/preempt_dev.inc).  Reservations are served (their virtual nodes carry their own job lists, cpp:6705), and
// so are partitions that share nodes (node-level job lists).
int cns_select_preempt(cns_handle* h, int64_t now, const cns_job_soa* jobs, const cns_preempt_soa* pre,
                       cns_placement_soa* out, cns_preempt_out* pout) {
  if (!h) return fail(h, CNS_ERR_INVALID_ARG, "cns_select_preempt: null handle");
  if (!pre || !pre->enabled) {
    if (int rc = cns_select(h, now, jobs, out)) return rc;
    cns_preempt::pass_through(jobs, pre, pout);   // the set passes through
    return CNS_OK;
  }
  if (const auto v = cns_preempt::check_select_preempt(h->have_nodes, h->rl_dev, jobs, pre, out, pout)) return fail(h, v.code, v.msg);
  struct PreCall { cns_engine* h; ~PreCall() { h->pre_call = false; } } pre_call{h};   // (run_resident_once notes it: cns_probe refuses such a state)
  h->pre_call = true;
  h->pre_t0 = std::chrono::steady_clock::now();
  h->rp_timing = cns_running_preempt_timing{};
  const u32 R = h->run.R;
  if (const auto v = cns_preempt::check_select_preempt_arrays(jobs->num_jobs, R, pre, pout)) return fail(h, v.code, v.msg);
  HIPCHK(h, hipSetDevice(h->device));
  if (int rc = cns_upload_jobs(h, jobs)) return rc;
  const cns_preempt::RunSide rs = cns_preempt::running_side(h->run.ent_job, h->run.rn_end, R, pre, now);
  // The device's running table carries the patched end times for THIS call only: whatever way the call ends, the resident
  // table goes back to the caller's end times (later cns_select / cns_run_resident calls reuse it).
  struct RestoreEnd {
    cns_engine* h; bool armed;
    ~RestoreEnd() {
      if (!armed) return;
      const std::string keep = h->err;   // the restore must not overwrite the call's own error
      if (upload(h, h->d_rn_end, h->run.rn_end) == CNS_OK) (void)hipStreamSynchronize(h->stream);
      h->err = keep;
    }
  } restore_end{h, false};
  if (rs.patched) { restore_end.armed = true; if (int rc = upload(h, h->d_rn_end, rs.ent_end)) return rc; }
  return pre_cycle(h, now, jobs, pre, out, pout, R, (u32)h->run.ent_job.size(), rs.set_in, "cns_select_preempt", [&](PreParams& Q) -> int {
    DevBuf* B = h->d_pre;
    if (int rc = upload_some(h, B[B_RNJOB], h->run.ent_job)) return rc;
    if (int rc = upload_some(h, B[B_ENTSLOT], h->run.ent_slot)) return rc;
    if (int rc = upload(h, B[B_RJQOS], rs.rj_qos)) return rc;
    if (int rc = upload(h, B[B_RJQP], rs.rj_qprio)) return rc;
    if (int rc = upload(h, B[B_RJSTART], rs.rj_start)) return rc;
    if (int rc = upload(h, B[B_RJEND], rs.rj_end)) return rc;
    if (int rc = upload(h, B[B_RJPRE], rs.rj_preempting)) return rc;
    if (int rc = upload(h, B[B_RJOFF], rs.rj_off)) return rc;
    if (int rc = upload(h, B[B_RJENT], rs.rj_ent)) return rc;
    Q.rn_job = B[B_RNJOB].as<u32>(); Q.ent_slot = B[B_ENTSLOT].as<u32>();
    Q.rj_qos = B[B_RJQOS].as<u32>(); Q.rj_qprio = B[B_RJQP].as<u32>(); Q.rj_start = B[B_RJSTART].as<i64>(); Q.rj_end = B[B_RJEND].as<i64>();
    Q.rj_preempting = B[B_RJPRE].as<uint8_t>(); Q.rj_off = B[B_RJOFF].as<u32>(); Q.rj_ent = B[B_RJENT].as<u32>();
    return 0;
  });
}

int cns_preempt_shape(uint32_t* sort_lanes, uint32_t* rank_sort_max, uint32_t* compact_records, uint32_t* cache_nodes, uint32_t* pool_nodes) {
  if (sort_lanes) *sort_lanes = kPreSortLanes;
  if (rank_sort_max) *rank_sort_max = kPreSortLanes * kPreSortChunks;
  if (compact_records) *compact_records = kPcCap;
  if (cache_nodes) *cache_nodes = kPreCacheN;
  if (pool_nodes) *pool_nodes = kPrePoolNodes;
  return CNS_OK;
}

int cns_select_shape(cns_select_shape_info* out) {
  if (!out) return CNS_ERR_INVALID_ARG;
  static_assert(w64::kWTRing == w32::kWTRing && w64::kWTRing == w16::kWTRing && w64::kWTRing == w8::kWTRing, "cns_select_shape: one task ring size for every build of k_wide");
  const cns_plan::Facts& F = plan_facts();   // the tiles as the launch plan has them
  cns_select_shape_info s{};
  s.tl_chunk = kTlChunk; s.tl_cap = kTlCap;
  s.multi_k = (u32)kMultiK; s.pipe_max_k = (u32)kPMaxK; s.max_upd = (u32)kMaxUpd; s.lds_heap = (u32)kLdsHeap; s.alloc_cache = (u32)kAllocCache;
  s.pipe_ring = kPRing; s.wide_task_ring = w64::kWTRing; s.pipe_xring = kPXRing; s.wide_window = w64::kWJ;
  s.sel_dip_max_npl = (u32)kSelDipMaxNpl;
  auto tiles = [](const cns_plan::Tiles& t, cns_tile_shape& o) {
    if (t.widths.size() > CNS_SHAPE_MAX_WIDTHS) return false;
    o.lanes = t.lanes; o.num_widths = (u32)t.widths.size();
    std::copy(t.widths.begin(), t.widths.end(), o.widths);
    return true;
  };
  bool ok = tiles(F.select, s.select) && tiles(F.pipe, s.pipe);
  for (u32 b = 0; b < 4; ++b) { ok = ok && tiles(F.wide[b].tiles, s.wide[b]); s.wide_waves[b] = F.wide[b].waves; }
  if (!ok) return CNS_ERR_UNSUPPORTED;   // (an experiment build with more tile widths than the record holds)
  *out = s;
  return CNS_OK;
}

int cns_serial_shape(cns_serial_shape_info* out) {
  if (!out) return CNS_ERR_INVALID_ARG;
  using W = w8::WideInfo;               // k_mem / k_giant are the 8-wave build's k_wide<1> in serial-only mode
  const cns_plan::Facts& F = plan_facts();
  static_assert(W::mem_slots == W::mem_lanes * 64u * W::mem_words && W::giant_mem_slots == W::mem_lanes * 64u * W::giant_mem_words, "cns_serial_shape: one bit per row of a scanner lane");
  cns_serial_shape_info s{};
  s.scan_lanes = W::mem_lanes; s.scan_trip_rows = W::mem_trip;
  s.mem_words = W::mem_words; s.giant_mem_words = W::giant_mem_words; s.mem_slots = F.mem_slots; s.giant_mem_slots = F.giant_mem_slots;
  s.helper_lanes = W::block; s.helper_trip_slots = W::giant_trip;
  s.helpers_max = F.giant_helpers_max; s.helper_budget = F.giant_helper_budget; s.helpers_min = cns_plan::kGiantMinHelpers;
  s.select_tile_slots = F.select.slots();
  *out = s;
  return CNS_OK;
}

int cns_get_partition_status(const cns_handle* h, uint8_t* status, uint32_t capacity) {
  if (!h || !status) return fail(const_cast<cns_handle*>(h), CNS_ERR_INVALID_ARG, "cns_get_partition_status: null argument");
  if (!h->have_nodes) return fail(const_cast<cns_handle*>(h), CNS_ERR_STATE, "cns_get_partition_status before cns_set_nodes");
  if (capacity < h->lay.Pu) return fail(const_cast<cns_handle*>(h), CNS_ERR_INVALID_ARG, "cns_get_partition_status: capacity below the number of partitions");
  for (u32 p = 0; p < h->lay.Pu; ++p) status[p] = h->lay.upart_refused[p];
  return CNS_OK;
}

int cns_device_results(cns_handle* h, void** dptr, uint64_t* bytes) {
  if (!h || !dptr || !bytes) return fail(h, CNS_ERR_INVALID_ARG, "cns_device_results: null argument");
  if (!h->have_jobs) return fail(h, CNS_ERR_STATE, "cns_device_results before cns_upload_jobs");
  *dptr = h->q.results.p;
  *bytes = h->q.ro.total;
  return CNS_OK;
}

int cns_get_timing(const cns_handle* h, cns_timing* t) {
  if (!h || !t) return CNS_ERR_INVALID_ARG;
  *t = h->timing;
  return CNS_OK;
}

int cns_debug_get_costs(cns_handle* h, double* out) {
  if (!h || !out) return fail(h, CNS_ERR_INVALID_ARG, "cns_debug_get_costs: null argument");
  if (!h->have_run) return fail(h, CNS_ERR_STATE, "cns_debug_get_costs before a successful run");
  HIPCHK(h, hipSetDevice(h->device));
  std::vector<double> c(std::max<u32>(h->rlay.S, 1));
  HIPCHK(h, hipMemcpy(c.data(), h->d_cost.p, (size_t)h->rlay.S * sizeof(double), hipMemcpyDeviceToHost));
  for (size_t i = 0; i < h->lay.orig_pos_slot.size(); ++i) out[i] = h->lay.orig_pos_slot[i] == kNone ? 0.0 : c[h->lay.orig_pos_slot[i]];
  return CNS_OK;
}

const char* cns_debug_last_kernel(const cns_handle* h) { return h ? h->last_kernel.c_str() : ""; }

uint32_t cns_debug_engine_partitions(const cns_handle* h) { return (h && h->have_nodes) ? h->rlay.P : 0u; }

int cns_debug_get_prof(cns_handle* h, uint64_t* out, uint32_t capacity) {
  // cycle counters of the last run, 32 per partition; all zero unless the library was built with -DCNS_PROF
  if (!h || !out) return fail(h, CNS_ERR_INVALID_ARG, "cns_debug_get_prof: null argument");
#ifndef CNS_DEBUG_FLUSH_LOG   // (the diagnostics build also reads them after a run that failed)
  if (!h->have_run) return fail(h, CNS_ERR_STATE, "cns_debug_get_prof before a successful run");
#endif
  HIPCHK(h, hipSetDevice(h->device));
  // behind them (from index 32 * P): 16 always-on protocol counter slots per partition of k_wide (every build; wide_kernel.inc kWs*)
#ifdef CNS_DEBUG_FLUSH_LOG
  const size_t n = std::min<size_t>((size_t)h->rlay.P * (32 + 16) + 2048, capacity);   // + the flush log of partition 0 (diagnostics build)
#else
  const size_t n = std::min<size_t>((size_t)h->rlay.P * (32 + 16), capacity);
#endif
  HIPCHK(h, hipMemcpy(out, h->d_prof.p, n * sizeof(u64), hipMemcpyDeviceToHost));
  return CNS_OK;
}

int cns_debug_get_timeline(cns_handle* h, uint32_t node, uint32_t capacity, uint32_t* len, int64_t* t,
                           int64_t* cpu_raw, uint64_t* mem, uint64_t* core_lo, uint64_t* core_hi, uint64_t* gres) {
  if (!h || !len) return fail(h, CNS_ERR_INVALID_ARG, "cns_debug_get_timeline: null argument");
  if (!h->have_run) return fail(h, CNS_ERR_STATE, "cns_debug_get_timeline before a successful run");
  if (node >= h->lay.N) return fail(h, CNS_ERR_INVALID_ARG, "cns_debug_get_timeline: node out of range");
  HIPCHK(h, hipSetDevice(h->device));
  const u32 slot = h->lay.node_slot[node];
  if (slot == kNone) { *len = 0; return CNS_OK; }  // not schedulable / in no partition: no NodeState (cpp:6595)
  const char* blk = h->d_blocks.as<char>() + (size_t)slot * kBlockStride;
  NodeHdr hd;
  HIPCHK(h, hipMemcpy(&hd, blk, sizeof hd, hipMemcpyDeviceToHost));
  const u32 n = hd.len;
  *len = n;
  u32 m = std::min(n, capacity);
  std::vector<TlMem> e(std::max<u32>(m, 1));
  if (m) HIPCHK(h, hipMemcpy(e.data(), blk + sizeof(NodeHdr), (size_t)m * sizeof(TlMem), hipMemcpyDeviceToHost));
  for (u32 i = 0; i < m; ++i) {
    t[i] = e[i].t; cpu_raw[i] = e[i].cpu; mem[i] = e[i].mem; core_lo[i] = e[i].clo; core_hi[i] = e[i].chi; gres[i] = e[i].gres;
  }
  return CNS_OK;
}

int cns_debug_get_timeline_cores(cns_handle* h, uint32_t node, uint32_t capacity, uint64_t* core_w2, uint64_t* core_w3) {
  if (!h || !core_w2 || !core_w3) return fail(h, CNS_ERR_INVALID_ARG, "cns_debug_get_timeline_cores: null argument");
  if (!h->have_run) return fail(h, CNS_ERR_STATE, "cns_debug_get_timeline_cores before a successful run");
  if (node >= h->lay.N) return fail(h, CNS_ERR_INVALID_ARG, "cns_debug_get_timeline_cores: node out of range");
  HIPCHK(h, hipSetDevice(h->device));
  const u32 slot = h->lay.node_slot[node];
  if (slot == kNone) return CNS_OK;
  const char* blk = h->d_blocks.as<char>() + (size_t)slot * kBlockStride;
  NodeHdr hd;
  HIPCHK(h, hipMemcpy(&hd, blk, sizeof hd, hipMemcpyDeviceToHost));
  const u32 m = std::min(hd.len, capacity);
  for (u32 i = 0; i < m; ++i) core_w2[i] = core_w3[i] = 0;
  if (!h->lay.wide_cores) return CNS_OK;   // (the TlExt array of a block is live only for snapshots with such core ids)
  std::vector<TlExt> e(std::max<u32>(m, 1));
  if (m) HIPCHK(h, hipMemcpy(e.data(), blk + sizeof(NodeHdr) + (size_t)kTlCap * sizeof(TlMem), (size_t)m * sizeof(TlExt), hipMemcpyDeviceToHost));
  for (u32 i = 0; i < m; ++i) { core_w2[i] = e[i].c2; core_w3[i] = e[i].c3; }
  return CNS_OK;
}

#include "priority_host.inc"
#include "limits_host.inc"
#include "steps_call.inc"
#include "probe_host.inc"
#include "resvq_host.inc"
#include "valid_host.inc"
#include "commit_host.inc"
#include "submit_host.inc"
#include "usage_host.inc"
#include "gate_host.inc"
#include "running_host.inc"
#include "running_preempt_host.inc"
#include "running_attrs_host.inc"
#include "running_amend_host.inc"

}  // extern "C"

#include "group_host.inc"
