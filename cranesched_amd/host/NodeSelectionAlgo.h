// C++ host side of the drop-in: the `INodeSelectionAlgo` plugin surface for CraneCtld's JobScheduler.
//
// The reference holds its node-selection algorithm as a concrete class
//     std::unique_ptr<SchedulerAlgo> m_node_selection_algo_;          src/CraneCtld/JobScheduler.h:1286
// built at src/CraneCtld/JobScheduler.cpp:158-159 and called once per cycle at :1441 through its single
// public method (JobScheduler.h:260-263):
//     void NodeSelect(const absl::Time& now,
//                     const std::vector<std::unique_ptr<RnJobInScheduler>>& running_jobs,
//                     const std::vector<std::unique_ptr<PdJobInScheduler>>& pending_jobs);
// `INodeSelectionAlgo` is that signature as an abstract base; `GpuNodeSelectionAlgo` implements it on top
// of the C ABI in include/crane_gpu/node_select.h, so swapping the make_unique at cpp:158-159 is the whole
// integration.  Struct and field names follow the reference (JobScheduler.h:57-170,
// PublicHeader.h:427-761) so that code written against CraneCtld's types reads the same here.
//
// abseil / protobuf / fpm are not available offline; their types are restated minimally:
//   absl::Time      -> crane::TimeSec   (int64 seconds; the path only uses whole seconds, cpp:1351)
//   cpu_t           -> crane::cpu_t     (int64 raw = value * 256, fpm::fixed<int64,__int128,8>)
//   CranedId/SlotId -> std::string, as in the reference
#pragma once
#include <cstdint>
#include <functional>
#include <list>
#include <map>
#include <memory>
#include <set>
#include <span>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <variant>
#include <vector>

struct cns_engine;
struct cns_group_info;
struct cns_submit_timing;
struct cns_usage_timing;

namespace crane {

using TimeSec = int64_t;
using job_id_t = uint32_t;
using CranedId = std::string;
using PartitionId = std::string;
using SlotId = std::string;

struct cpu_t {  // fpm::fixed<int64_t, __int128, 8>
  int64_t raw = 0;
  cpu_t() = default;
  explicit cpu_t(int v) : raw(static_cast<int64_t>(v) * 256) {}
  explicit cpu_t(double v) : raw(static_cast<int64_t>(v * 256.0 + (v >= 0 ? 0.5 : -0.5))) {}
  static cpu_t from_raw(int64_t r) { cpu_t c; c.raw = r; return c; }
  explicit operator double() const { return static_cast<double>(raw) / 256.0; }
  bool operator==(const cpu_t& o) const { return raw == o.raw; }
};

struct GresCount {  // PublicHeader.h:505-523
  uint64_t total{0};
  std::unordered_map<std::string /*type*/, uint64_t> specified;
};
using GresMap = std::unordered_map<std::string /*name*/, GresCount>;

struct ResourceView {  // PublicHeader.h:695-761 (fields that reach the path)
  cpu_t cpu_count;
  uint64_t memory_bytes{0};
  uint64_t memory_sw_bytes{0};
  GresMap gres_map;
};

struct CpuSet {  // PublicHeader.h:555-573
  std::set<uint32_t> core_ids;
  cpu_t cpu_count;
};
using TypeSlotsMap = std::unordered_map<std::string /*type*/, std::set<SlotId>>;
using DedicatedResourceInNode = std::unordered_map<std::string /*name*/, TypeSlotsMap>;

struct ResourceInNodeV3 {  // PublicHeader.h:586-639
  CpuSet cpu_set;
  uint64_t memory_bytes{0};
  uint64_t memory_sw_bytes{0};
  DedicatedResourceInNode gres;
};
using ResourceV3 = std::unordered_map<CranedId, ResourceInNodeV3>;  // EachNodeResMap()

struct RnJobInScheduler {  // JobScheduler.h:57-90
  job_id_t job_id{0};
  std::string qos;                    // h:68: read by TryPreempt_ through NodeState::qos_job_map
  PartitionId partition_id;
  std::string reservation;
  TimeSec start_time{0};
  TimeSec end_time{0};
  ResourceV3 allocated_res;
  // read by MultiFactorPriority (JobScheduler.cpp:7692-7746)
  std::string account;
  uint32_t qos_priority{0};
  uint32_t partition_priority{0};
  uint32_t node_num{0};               // uninitialised in the reference (h:70,76-89); here: allocated_res.size() when 0
  ResourceView allocated_res_view;    // cpu_count + memory_bytes of the whole allocation
};

struct PdJobInScheduler;
using PreemptedJob = std::variant<PdJobInScheduler*, RnJobInScheduler*>;   // JobScheduler.h:124-126

struct PdJobInScheduler {  // JobScheduler.h:92-170
  job_id_t job_id{0};
  int64_t time_limit{0};  // absl::Duration, whole seconds
  PartitionId partition_id;
  std::string reservation;
  ResourceView req_node_res_view;
  ResourceView req_task_res_view;
  uint32_t node_num{1};
  uint32_t ntasks_per_node_min{1};
  uint32_t ntasks_per_node_max{1};
  uint32_t ntasks{1};
  bool exclusive{false};
  std::unordered_set<std::string> included_nodes;
  std::unordered_set<std::string> excluded_nodes;
  // results (JobScheduler.h:117-133)
  std::unordered_map<CranedId, uint32_t> craned_id_to_task_num;
  TimeSec start_time{0};
  TimeSec end_time{0};
  ResourceV3 allocated_res;
  std::vector<CranedId> craned_ids;
  std::string reason;
  std::vector<PreemptedJob> preempted_jobs;   // result of TryPreempt_ (JobScheduler.cpp:6490-6496), push_back order
  bool is_scheduled() const { return reason.empty(); }
  // licenses (JobScheduler.h:141-146; LicenseManager::CheckLicenseCountSufficient, LicenseManager.cpp:167-221)
  std::vector<std::pair<std::string, uint32_t>> req_licenses;   // (license id, count), request order
  bool is_license_or{false};
  std::unordered_map<std::string, uint32_t> actual_licenses;    // result
  // read / written by MultiFactorPriority (JobScheduler.cpp:7616, :7664-7690, :7759-7767)
  TimeSec submit_time{0};
  std::string account;
  uint32_t qos_priority{0};
  uint32_t partition_priority{0};
  double priority{0.0};               // cached across cycles: 0.0 = compute (cpp:7616)
  ResourceView req_total_res_view;    // req_node * node_num + req_task * ntasks (cpp:7156)
  // read by the commit loop's run-limit check (AccountMetaContainer::CheckAndMallocMetaResource); the account chain
  // (job.account_chain, JobScheduler.h:108) is derived from AccountMetaSnapshot::account_parent
  std::string username;
  std::string qos;
};

// What NodeSelect's prologue reads from g_meta_container (JobScheduler.cpp:6563-6617): per craned its
// res_total, alive/drain, and the partition -> craned ids map.  In CraneCtld the adapter fills this from
// CranedMetaContainer (src/CraneCtld/Node/CranedMetaContainer.h:116-120, NodeDefs.h:59-81) while holding
// the same locks the reference takes.
struct CranedMeta {
  CranedId craned_id;
  ResourceInNodeV3 res_total;
  bool alive{true};
  bool drain{false};
};
// ResvMeta as NodeSelect reads it (JobScheduler.cpp:6627-6679): window and the reserved resources per node.
struct ResvMeta {
  std::string name;          // ResvId
  TimeSec start_time{0};
  TimeSec end_time{0};
  ResourceV3 res_total;      // EachNodeResMap()
};
struct ClusterSnapshot {
  std::vector<CranedMeta> craned_metas;                                   // dense order = canonical tie-break order
  std::vector<std::pair<PartitionId, std::vector<CranedId>>> partitions;  // PartitionMeta::craned_ids
  std::vector<ResvMeta> reservations;                                     // g_meta_container->GetResvMetaMapPtr(); vector order = canonical order
  // g_config.Preempt.PreemptType != NONE (PREEMPT_QOS): NodeSelect calls LocalScheduler::TryPreempt_ (JobScheduler.cpp:
  // 6140-6143) with the preempt lists of the QoS table (cpp:6532-6543: Qos::preempt of every pending job's qos).  Served by
  // cns_select_preempt (include/crane_gpu/preempt.h) through NodeSelect(now, running_jobs, pending_jobs) — also together
  // with reservations and with partitions that share nodes.  The mirror-fed form NodeSelect(now, pending_jobs) has no
  // RnJobInScheduler objects to hand back in preempted_jobs and is refused for such a snapshot (CNS_ERR_STATE).
  bool preempt_enabled{false};
  std::unordered_map<std::string, std::vector<std::string>> qos_preempt;   // qos name -> Qos::preempt
};

// ---- what the commit loop's run-limit admission reads (JobScheduler.cpp:1557-1573) -----------------------------
// Qos (src/CraneCtld/Account/AccountDefs.h:27-49), the fields CheckRunLimits_ reads
struct Qos {
  uint32_t max_jobs_per_user{UINT32_MAX};
  uint32_t max_jobs_per_account{UINT32_MAX};
  uint32_t max_jobs{UINT32_MAX};
  cpu_t max_cpus_per_user{cpu_t::from_raw(int64_t{1} << 53)};   // kUnlimitedCpu
  int64_t max_wall{0};                                          // absl::Duration seconds, 0 = unlimited
  ResourceView max_tres, max_tres_per_user, max_tres_per_account;
  // the submit side (TryMallocMetaSubmitResource, AccountMetaContainer.cpp:75-153); the defaults mean "unlimited / flag off"
  uint32_t max_submit_jobs_per_user{UINT32_MAX};
  uint32_t max_submit_jobs_per_account{UINT32_MAX};
  uint32_t max_submit_jobs{UINT32_MAX};
  bool deny_on_limit{false};                                    // flags[QosFlags::DenyOnLimit]
  int64_t max_time_limit_per_job{315576000000};                 // absl::Duration seconds; kJobMaxTimeLimitSec
  Qos();
};
struct PartitionResourceLimit {  // AccountDefs.h:163-175
  ResourceView max_tres;
  uint32_t max_jobs{UINT32_MAX};
  int64_t max_wall{0};
  // the submit side (CheckSubmitLimits_, AccountMetaContainer.cpp:715-749,784-819)
  ResourceView max_tres_per_job;
  uint32_t max_submit_jobs{UINT32_MAX};
  int64_t max_wall_duration_per_job{315576000000};              // the reference sets it from the database; kJobMaxTimeLimitSec = no cap
  PartitionResourceLimit();
};
struct MetaResource {  // AccountMetaContainer.h:30-35
  ResourceView resource;
  uint32_t jobs_count{0};
  uint32_t submit_jobs_count{0};   // counted at submit time (h:33); the run-limit admission neither reads nor changes it
  int64_t wall_time{0};
};
struct MetaResourceStat {  // AccountMetaContainer.h:62-80
  std::unordered_map<std::string /*qos*/, MetaResource> qos_to_resource_map;
  std::unordered_map<std::string /*account*/, std::unordered_map<PartitionId, MetaResource>> account_to_partition_to_resource_map;  // users
  std::unordered_map<PartitionId, MetaResource> partition_to_resource_map;                                                          // accounts
};
// The state of AccountManager + AccountMetaContainer the check reads, copied by the caller under the locks the
// reference takes (AccountMetaContainer.cpp:204-207).
struct AccountMetaSnapshot {
  std::unordered_map<std::string, Qos> qos;                                              // GetExistedQosInfo
  std::unordered_map<std::string, std::string> account_parent;                           // Account::parent_account, "" = root
  std::unordered_map<std::string, std::unordered_map<PartitionId, PartitionResourceLimit>> account_partition_limits;  // Account::partition_to_limit_map
  // User::account_to_attrs_map: the accounts of a user, each with its partition_to_limit_map
  std::unordered_map<std::string, std::unordered_map<std::string, std::unordered_map<PartitionId, PartitionResourceLimit>>> user_accounts;
  std::unordered_map<std::string, MetaResourceStat> user_meta;     // m_user_meta_map_
  std::unordered_map<std::string, MetaResourceStat> account_meta;  // m_account_meta_map_
  std::unordered_map<std::string, MetaResource> qos_meta;          // m_qos_meta_map_
};

// ---- step scheduling (JobInCtld::SchedulePendingSteps, CtldPublicDefs.cpp:2038-2159) ---------------------------
// The CommonStepInCtld fields that function reads and writes.
struct StepInScheduler {
  uint32_t step_id{0};
  ResourceView req_node_res_view, req_task_res_view;
  uint32_t node_num{1}, ntasks{1}, ntasks_per_node_min{1}, ntasks_per_node_max{1};
  std::unordered_set<std::string> included_nodes, excluded_nodes;
  // results (:2129-2135)
  bool scheduled{false};
  std::vector<CranedId> craned_ids;                                   // in the order the nodes were handed tasks
  ResourceV3 allocated_res;                                           // step_alloc_res
  std::unordered_map<CranedId, std::set<uint32_t>> craned_task_map;   // task ids per node
  std::unordered_map<uint32_t, ResourceInNodeV3> task_res_map;        // per task id
};
// One running job with pending steps: its step_res_avail_ (updated in place) and pending_step_ids_ in queue order.
struct JobStepQueue {
  job_id_t job_id{0};
  ResourceV3* step_res_avail{nullptr};
  std::vector<StepInScheduler*> pending_steps;
};

// License (LicenseManager: total, used, reserved, last_deficit as read at LicenseManager.cpp:188-189,203-204)
struct License {
  uint32_t total{0}, used{0}, reserved{0}, last_deficit{0};
};

// g_config.PriorityConfig, CtldPublicDefs.h:162-174
struct PriorityConfig {
  bool FavorSmall{true};
  uint64_t MaxAge{14 * 24 * 3600};
  uint32_t WeightAge{500}, WeightFairShare{10000}, WeightJobSize{0}, WeightPartition{1000}, WeightQoS{1000000};
};

// JobScheduler.h:174-181: what NodeSelect calls at JobScheduler.cpp:6735 before its ordered loop.
class IPrioritySorter {
 public:
  virtual ~IPrioritySorter() = default;
  virtual void GetOrderedJobPtrVec(const TimeSec& now, const std::vector<std::unique_ptr<PdJobInScheduler>>& pending_jobs,
                                   const std::vector<std::unique_ptr<RnJobInScheduler>>& running_jobs, size_t limit,
                                   std::vector<PdJobInScheduler*>& job_ptr_vec) = 0;
};

// MultiFactorPriority (JobScheduler.h:203-231, JobScheduler.cpp:7606-7819) on the MI355X: bounds, service
// values, priorities and the ordering run on the device (include/crane_gpu/priority.h).  Writes job->priority,
// fills job_ptr_vec with the first `limit` jobs by descending priority (ties: input order) and marks the rest
// "Priority" (cpp:7625-7630).  On an engine error the vector keeps input order and LastError() says why.
// A sorter built over a GpuNodeSelectionAlgo BORROWS that object's engine (the algorithm object must outlive it): when the algorithm
// runs with resident running and its device ledger carries the attribute columns (include/crane_gpu_running/running_attrs.h:
// SeedRunning / AdvanceRunning hand them in), the running side is read from the ledger — ledger row i is running job i — and the
// CONTENTS of `running_jobs` are not touched (the vector may be empty).  Otherwise it behaves as the sorter with a handle of its own.
class GpuNodeSelectionAlgo;
class GpuMultiFactorPriority final : public IPrioritySorter {
 public:
  explicit GpuMultiFactorPriority(const PriorityConfig& cfg, int device = 0);
  GpuMultiFactorPriority(const PriorityConfig& cfg, GpuNodeSelectionAlgo* algo);
  ~GpuMultiFactorPriority() override;
  GpuMultiFactorPriority(const GpuMultiFactorPriority&) = delete;
  GpuMultiFactorPriority& operator=(const GpuMultiFactorPriority&) = delete;
  void GetOrderedJobPtrVec(const TimeSec& now, const std::vector<std::unique_ptr<PdJobInScheduler>>& pending_jobs,
                           const std::vector<std::unique_ptr<RnJobInScheduler>>& running_jobs, size_t limit,
                           std::vector<PdJobInScheduler*>& job_ptr_vec) override;
  bool Ok() const { return status_ == 0; }
  const std::string& LastError() const { return error_; }

 private:
  PriorityConfig cfg_;
  cns_engine* h_{nullptr};
  GpuNodeSelectionAlgo* algo_{nullptr};   // the owner of h_ when it is borrowed
  int status_{0};
  std::string error_;
};

class INodeSelectionAlgo {
 public:
  virtual ~INodeSelectionAlgo() = default;
  virtual void NodeSelect(const TimeSec& now,
                          const std::vector<std::unique_ptr<RnJobInScheduler>>& running_jobs,
                          const std::vector<std::unique_ptr<PdJobInScheduler>>& pending_jobs) = 0;
};

// MI355X implementation.  It has no CPU path of its own: on an engine-level failure (no GPU, unsupported input) every pending job
// is left unscheduled with reason "GpuEngineError", Ok() / LastStatus() / LastError() say why, and the CALLER decides — INTEGRATION.md
// §3 wires the reference's own SchedulerAlgo behind this class for exactly that case (two lines in JobScheduler's constructor).
class GpuNodeSelectionAlgo final : public INodeSelectionAlgo {
 public:
  explicit GpuNodeSelectionAlgo(int device = 0, uint64_t scheduled_batch_size = 0);
  // Several devices of one node: the groups of partitions connected through shared nodes are dealt over them (group g -> devices[g % N]),
  // every device runs its shard of the ordered queue on its own host thread, ONE all-gather (RCCL) merges the packed results
  // (include/crane_gpu/node_select.h, "several devices").  {d} is the one-device form.
  explicit GpuNodeSelectionAlgo(const std::vector<int>& devices, uint64_t scheduled_batch_size = 0);
  // What lies outside the engine's limits (a node with a core id >= 256, GRES classes / slots beyond the 64-bit mask, the 65th distinct
  // res_total record, a group of partitions wider than the widest tile — the reference bounds none of it, PublicHeader.h:555-573,427-494)
  // refuses ONLY the group of partitions it touches: their jobs leave NodeSelect with reason "GpuEngineRefused" and nothing else set, every
  // other partition is served.  RefusedJobs(): exactly those jobs of the last cycle, in its order — the caller's CPU SchedulerAlgo takes
  // them.  RefusedPartitions(): which partitions of the snapshot, and UnsupportedNodes(): how many nodes caused it.
  const std::vector<const PdJobInScheduler*>& RefusedJobs() const;
  std::vector<PartitionId> RefusedPartitions() const;
  size_t UnsupportedNodes() const;
  size_t NumDevices() const;
  bool LastGroupInfo(cns_group_info* out) const;   // false on one device
  ~GpuNodeSelectionAlgo() override;
  GpuNodeSelectionAlgo(const GpuNodeSelectionAlgo&) = delete;
  GpuNodeSelectionAlgo& operator=(const GpuNodeSelectionAlgo&) = delete;

  // Per-cycle snapshot (the reference re-reads the meta container inside NodeSelect; here the caller
  // hands the snapshot over before the call).
  void SetClusterSnapshot(const ClusterSnapshot& snap);
  // Incremental form for what changes between cycles without changing the node set (CranedMetaContainer::CranedUp /
  // CranedDown, CranedMetaContainer.cpp:26-122, and the drain flag): flips the node's "schedulable" bit
  // (alive && !drain, JobScheduler.cpp:6595) and re-sends the packed tables; the snapshot's dense indices, the
  // reservation tables and the cached running allocations stay valid.  SetClusterSnapshot is only needed again when
  // nodes, partitions, res_total or reservations change.
  void SetCranedState(const CranedId& craned_id, bool alive, bool drain);
  // Optional: the sorter NodeSelect consults first (SchedulerAlgo's ctor argument, JobScheduler.h:247);
  // nullptr = BasicPriority (input order, JobScheduler.h:185-200).  Not owned.
  void SetPrioritySorter(IPrioritySorter* sorter) { sorter_ = sorter; }
  // Default: jobs that did not start now (pending reason set) get reason, start_time and end_time only — all the commit
  // loop reads of them (JobScheduler.cpp:1503-1510).  SetFullWriteBack(true) also fills craned_ids / allocated_res of the
  // jobs NodeSelect backfilled for later, exactly as the reference's NodeSelect leaves them.
  void SetFullWriteBack(bool full);
  // Deferred write-back: a job that starts now leaves NodeSelect with reason, start_time, end_time and craned_ids — everything the
  // commit loop reads up to the run-limit admission (JobScheduler.cpp:1503-1573); MaterializeAllocation(job) then fills its
  // craned_id_to_task_num / allocated_res (exactly what the full write-back builds) for the jobs that ARE launched (:1590-1600),
  // from the packed placements the adapter keeps.  0.39 -> 0.1 us per started job in NodeSelect; false: the job was not placed.
  void SetDeferredWriteBack(bool deferred);
  // Host threads for the two per-job loops of a cycle (packing the pending jobs, the write-back): default 1, like the reference's
  // single ScheduleThread; jobs are independent there, so n threads take n slices of the ordered vector.  The engine's own pass over the
  // queue inside cns_select follows the same number (cns_set_host_threads on every device's engine); without a call it keeps its
  // default (CNS_HOST_THREADS from the environment, else up to 16 threads for queues of 32 768 jobs and more).
  void SetHostThreads(int n);
  bool MaterializeAllocation(PdJobInScheduler& job);
  // The cycle's license table for the pre-pass NodeSelect runs between ordering and selection
  // (g_license_manager->CheckLicenseCountSufficient, JobScheduler.cpp:6739; LicenseManager.cpp:167-221): a tiny
  // sequential counter pass over the ordered jobs, done on the host; jobs it rejects get reason "License" and are
  // not given to the device.  Empty table + no requests = no-op.
  void SetLicenses(std::unordered_map<std::string, License> licenses) { licenses_ = std::move(licenses); }
  // ... the pass itself (host-only; NodeSelect calls it with the table of SetLicenses and the sorter's order)
  static void CheckLicenseCountSufficient(const std::unordered_map<std::string, License>& licenses, const std::vector<PdJobInScheduler*>& ord);

  void NodeSelect(const TimeSec& now, const std::vector<std::unique_ptr<RnJobInScheduler>>& running_jobs,
                  const std::vector<std::unique_ptr<PdJobInScheduler>>& pending_jobs) override;

  // ---- what-if probes (include/crane_gpu_probe/probe.h; the reference has no such call) -------------------------------------
  // "When and where would THIS job run if it were submitted now?" for every job of `jobs`, independently of each other, against the
  // final state of the last NodeSelect: per job exactly what that cycle would have written for it behind the last job its ordered
  // loop took — and nothing is committed, the cycle's own results (MaterializeAllocation, the wire emission, RefusedJobs) stay.
  // The jobs are packed by the packer of the cycle (same name tables, same GRES class order, unknown include names as in NodeSelect;
  // no sorter, no license pre-pass: probes are questions, not the queue).  Written into the objects handed in, and nowhere else:
  // reason, start_time, end_time, craned_ids, craned_id_to_task_num, allocated_res — always in full, whatever write-back mode the
  // cycle runs in; a job that comes with a reason keeps it and is not asked.  On an engine error (no cycle yet, a cycle with
  // preemption, no device) the jobs without a reason get "GpuEngineError" and Ok() / LastStatus() / LastError() say why; nothing is
  // thrown.  One device only: an algorithm object built over several devices refuses with CNS_ERR_UNSUPPORTED.
  void ProbeStart(const std::vector<PdJobInScheduler*>& jobs);

  // ---- reservation what-ifs (include/crane_gpu_resv/resv_probe.h) ----------------------------------------------------------------
  // The node walk of JobScheduler::CreateResv_ (JobScheduler.cpp:4383-4419) for every request at once, against the running set the
  // adapter packed last (NodeSelect / the mirror) and the reservations of the snapshot: which of `craned_ids` could the reservation
  // take, in list order — at `start`, or with find_earliest at the first start >= `start` at which `node_num` of them are free for
  // `duration` (node_num 0: all of the list, :4357-4358).  Nothing is created.  Per request what CreateResv_'s error text is built
  // from (:4421-4437): ok, the start the answer holds for, the chosen nodes, and the conflicted / not-found nodes of the WHOLE list at
  // that start (the reference stops at the node_num-th free node; its lists are the prefix up to there).  A request whose end is not
  // after `now` (:4323) comes back with in_the_past and nothing else.  On an engine error (no device, no snapshot, a node named twice
  // in one list, duration <= 0) the result is empty and Ok() / LastStatus() / LastError() say why; nothing is thrown.
  // The engine's per-node tables (cns_resvq_set_state) are rebuilt only when the running set or the snapshot was packed anew since the
  // last call.  As in a cycle, a running job whose reservation name the snapshot does not know is not part of the packed running set.
  // With resident running on nothing packs the running set behind SeedRunning: the running side then comes from the device ledger
  // (cns_resvq_set_state_resident) and is taken again behind SeedRunning, AdvanceRunning, AmendRunning and a new snapshot.
  struct ResvRequest {
    TimeSec start{0};
    int64_t duration{0};
    uint32_t node_num{0};
    std::vector<CranedId> craned_ids;
    bool find_earliest{false};
  };
  struct ResvAnswer {
    bool ok{false}, in_the_past{false};
    TimeSec start{0};
    std::vector<CranedId> chosen, conflicted, not_found;
  };
  std::vector<ResvAnswer> QueryReservation(const TimeSec& now, std::span<const ResvRequest> requests, double* kernel_ms = nullptr);

  // ---- validity of a batch of submissions (include/crane_gpu_valid/validity.h) -----------------------------------------------------
  // The partition checks of JobScheduler::CheckJobValidity (JobScheduler.cpp:7262-7374) for every job at once: can the partition the
  // job names EVER run it, and on how many of its nodes — the call at :371 batched over the recovered queue, or a bulk re-check after a
  // partition changed.  The jobs go through the packer of the cycle; nothing of a job is written.  Per job the engine's code
  // (cns_valid_code), the number of nodes of the partition that pass the walk's test (the full count, :7364's break is not taken) and
  // the CraneErrCode NAME the reference returns there: "" when the job is valid, ERR_INVALID_PARAM (:7264,:7268,:7312,:7347; also a
  // request whose arithmetic overflows), ERR_INVALID_PARTITION (an unknown partition: the reference refuses it before this function,
  // :7022), ERR_NO_RESOURCE (:7296), ERR_INVALID_NODE_NUM (:7304), ERR_NO_ENOUGH_NODE (:7373).  `refused`: the partition lists a node
  // this adapter could not express (UnsupportedNodes()): nothing was decided, ask the CPU code.
  // What the snapshot packs as res_total of a node that is down or drained is its res_total, unchanged: SetCranedState only flips the
  // schedulable flag, as CranedDown leaves res_total alone (CranedMetaContainer.cpp:83-122) — and the walk (:7354-7357) reads exactly that,
  // whether the node is alive or not; the check does not read the flag.
  // The packer saturates GRES counts (a total at 255, a specified count at 127; an unknown name or type: 255): such a request is never
  // valid, but where the reference says ERR_NO_RESOURCE for a count between the saturation and the partition's total this says
  // ERR_NO_ENOUGH_NODE.  The time limit, the array spec, the deadline and the reservation's partition / account / user lists
  // (:7225-7272,:7317-7336) stay with the caller.  false on an engine error (no device, no snapshot, several devices: CNS_ERR_UNSUPPORTED, as
  // ProbeStart): `out` is empty and Ok() / LastStatus() / LastError() say why; nothing is thrown.
  struct ValidityAnswer {
    uint8_t code{0};               // cns_valid_code
    uint32_t eligible{0};
    const char* crane_err{""};     // CraneErrCode name, "" = valid (or refused)
    bool refused{false};
  };
  bool CheckJobValidity(const std::vector<const PdJobInScheduler*>& jobs, std::vector<ValidityAnswer>* out, double* kernel_ms = nullptr);

  // ---- the commit loop's checks behind NodeSelect (include/crane_gpu_commit/commit_check.h) ----------------------------------------
  // The resource-reduce check (JobScheduler.cpp:1464-1540) and the preempted-still-alive check (:1542-1555) for every job of the last
  // NodeSelect at once, in front of the loop at :1492.  Inputs in the reference's own shapes:
  //   events         what g_meta_container->LockAndGetResReduceEvents() holds (:1468): per event a ResvId, or (time, craned ids);
  //   resv_now       GetResvMetaPtr(name) NOW (:1523): nullptr = deleted, else its end_time and craned_ids;
  //   running_alive  the ids of m_running_job_map_ NOW (:1546) — only the victims of the last cycle are looked up;
  //   pending_alive  the ids still in m_pending_job_map_ (:1493).
  // They are packed to dense indices with the tables of the last NodeSelect / SetClusterSnapshot: a craned name the snapshot does not know
  // touches no placed job and is dropped; so is a reservation name the cycle did not know (its jobs carry "Reservation Not Found").  The
  // preempted lists of the last cycle with preemption go along.  The reference's string is written into job->reason exactly where
  // :1518-1552 does ("Resource changed", "Reservation deleted", "Resource", "Reservation changed", "Waiting for Preemption"); a job that
  // is gone is reported and not written, a job the cycle left a reason keeps it.  CheckAndMallocMetaResource skips a job whose reason is
  // not empty, so calling this first makes the batched admission exact.  `codes` (may be null): cns_commit_code per job, in the order of
  // the last cycle (LastOrder()).  Licenses (:1557-1563) stay with the caller.  false on an engine error (no device, no cycle yet,
  // several devices: CNS_ERR_UNSUPPORTED): nothing is written and Ok() / LastStatus() / LastError() say why; nothing is thrown.
  struct ResvMetaNow {
    TimeSec end_time{0};
    std::vector<CranedId> craned_ids;
  };
  struct ResReduceEvent {   // CranedMetaContainer.h: ResReduceEvent::affected_resources
    std::variant<std::string, std::pair<TimeSec, std::vector<CranedId>>> affected_resources;
  };
  static constexpr TimeSec kInfinitePast = INT64_MIN;   // absl::InfinitePast(): CranedDown / drain events
  bool CommitCheck(const std::vector<ResReduceEvent>& events, const std::function<const ResvMetaNow*(const std::string&)>& resv_now,
                   const std::unordered_set<job_id_t>& running_alive, const std::unordered_set<job_id_t>& pending_alive,
                   std::vector<uint8_t>* codes = nullptr, double* kernel_ms = nullptr);

  // ---- the pending gate in front of NodeSelect (include/crane_gpu_gate/pending_gate.h) ------------------------------------------------
  // The dependency-event drain (JobScheduler.cpp:1353-1372) and Phase 1 (:1374-1413) of ScheduleThread_ for the whole pending map at
  // once: which jobs reach NodeSelect this cycle.  Inputs in the reference's own shapes:
  //   jobs     one entry per job of m_pending_job_map_, in any order: Held() as the caller evaluated it, begin_time, a pointer to the
  //            job's DependenciesInJob (CtldPublicDefs.h:454-469; null: the struct's defaults, no dependencies) and, for an array parent,
  //            what PrepareParentForMaterialization and SpawnBlockReason read (Array.cpp:683-699, :236-259);
  //   events   what m_dependency_event_queue_ handed out (:1357), in queue order.
  // The adapter sorts the jobs by id (the btree order of :1377) and every dependency list by dependee, calls cns_gate_pending, and
  // then leaves every DependenciesInJob as the reference's UpdateDependency calls would: ready_time folded, the applied entries erased
  // (CtldPublicDefs.cpp:154-159).  Feeding the same structs into the next cycle's call therefore continues where the reference's
  // JobInCtld would.  Times are whole seconds (fractional times rounded UP, pending_gate.h "Time domain"); kInfiniteFuture /
  // kInfinitePast are absl::InfiniteFuture() / InfinitePast().
  // out->code[i] / reason[i]: cns_gate_code and the pending_reason string of jobs[i]; out->pending: indices into `jobs` in ascending
  // job id, the pending_jobs vector of :1375-1413; materializes_array_child alongside (:1406).  Held() itself, the array manager's
  // bookkeeping, the construction of PdJobInScheduler and TriggerDependencyEvents stay with the caller.  Needs a device, no snapshot.
  // false on an engine error (no device, two jobs with one id or another refused input): `out` is empty, no DependenciesInJob is written
  // and Ok() / LastStatus() / LastError() say why; nothing is thrown.
  struct DependenciesInJob {   // CtldPublicDefs.h:454-469
    std::unordered_map<job_id_t, std::pair<int, uint64_t>> deps;   // dependee -> (crane::grpc::DependencyType, delay seconds)
    bool is_or{false};
    TimeSec ready_time{INT64_MIN};
  };
  struct ArrayParentGate {
    bool has_meta{true};               // FindMeta_(parent.JobId()) != nullptr        Array.cpp:686
    bool has_parent{true};             // parent_job_ != nullptr                      Array.cpp:237
    bool materialization_complete{false};
    bool cancel_requested{false};
    TimeSec deadline_time{INT64_MAX};
    bool has_next_task{true};          // NextMaterializableTaskId().has_value()      Array.cpp:249
    uint64_t running_children{0};      // RunningChildCount()
    uint64_t run_limit{UINT64_MAX};    // ArrayUtil::EffectiveRunLimit(array_spec)
  };
  struct PendingGateJob {
    job_id_t job_id{0};
    bool held{false};
    TimeSec begin_time{INT64_MIN};
    DependenciesInJob* dependencies{nullptr};
    bool is_array_parent{false};
    ArrayParentGate array;
  };
  struct DependencyEvent {   // JobScheduler.h: DependencyEvent
    job_id_t dependent_job_id{0}, dependee_job_id{0};
    TimeSec event_time{0};
  };
  struct PendingGateResult {
    std::vector<uint8_t> code;                       // [jobs.size()] cns_gate_code
    std::vector<const char*> reason;                 // [jobs.size()] job->pending_reason
    std::vector<uint32_t> pending;                   // indices into jobs: pending_jobs, in its order
    std::vector<uint8_t> materializes_array_child;   // [pending.size()]
    uint64_t counts[16]{};                           // jobs per code
    uint64_t ev_stats[3]{};                          // events applied, without their pending job, without their dependency
    double kernel_ms{0.0};
  };
  static constexpr TimeSec kInfiniteFuture = INT64_MAX;   // absl::InfiniteFuture()
  bool BuildPendingQueue(TimeSec now, const std::vector<PendingGateJob>& jobs, const std::vector<DependencyEvent>& events, PendingGateResult* out);

  // ---- the submit limits over a batch of submissions (include/crane_gpu_submit/submit_limits.h) -----------------------------------------
  // AccountMetaContainer::TryMallocMetaSubmitResource + MallocMetaSubmitResource (AccountMetaContainer.cpp:75-153, the call at
  // JobScheduler.cpp:3465-3476) for every request, IN THE ORDER GIVEN (arrival order): request i sees the submit counts as requests 0..i-1
  // left them.  The jobs go through the packer of the cycle (its partition and GRES name tables); `meta` is packed to dense indices as
  // CheckAndMallocMetaResource packs it, with the submit-side fields of Qos / PartitionResourceLimit, MetaResource::submit_jobs_count and
  // "the user / account / QoS has a record" (user_meta / account_meta / qos_meta contain the name).  Per request the engine's code
  // (cns_submit_code: the first failing check in the reference's order), the CraneErrCode NAME the reference returns there ("SUCCESS" when
  // admitted; ERR_INVALID_PARAM for count == 0, JobScheduler.cpp:3466, and for a request whose arithmetic overflows) and the time limit
  // after :118-119.  A request with `skip` set is not looked at (it failed CheckJobValidity or an earlier check): "" and
  // CNS_SUBMIT_NOT_CANDIDATE; an unknown user, account, QoS or partition — lookups that stay with the caller, :3461-3463, :85-95 — comes back
  // as ERR_INVALID_USER / ERR_INVALID_ACCOUNT / ERR_INVALID_QOS / ERR_INVALID_PARTITION with the same code and nothing checked.
  // Written: `meta`'s submit_jobs_count of every record an admitted request touched and the records an admission created
  // (DoMallocResource_, :1067-1124); jobs_count, resource and wall_time stay.  An admitted job's time_limit is rewritten as :119 does.
  // UserAddJob (:3476) and qos_priority (:116) stay with the caller; the frees are ReleaseMetaResources.  false on an engine error (no device, no snapshot, several
  // devices: CNS_ERR_UNSUPPORTED, counts that could pass UINT32_MAX, a chain of more than 6 accounts): `out` is empty, nothing is written and
  // Ok() / LastStatus() / LastError() say why; nothing is thrown.
  struct SubmitRequest {
    PdJobInScheduler* job{nullptr};
    uint32_t count{1};             // QosSubmitReserveCount(job): an array job's children, else 1
    bool skip{false};
  };
  struct SubmitAnswer {
    uint8_t code{0};               // cns_submit_code
    const char* crane_err{""};     // CraneErrCode name
    int64_t time_limit{0};
  };
  bool CheckSubmitLimits(const std::vector<SubmitRequest>& requests, AccountMetaSnapshot* meta, std::vector<SubmitAnswer>* out,
                         cns_submit_timing* timing = nullptr);

  // ---- releases and charges on the usage records (include/crane_gpu_usage/usage.h) -----------------------------------------------------
  // AccountMetaContainer::DoFreeResource_ (AccountMetaContainer.cpp:1126-1208) / DoMallocResource_ (:1067-1124) for every delta IN THE
  // ORDER GIVEN: one delta per Free... / Malloc... call of the reference, built by the maker named after that call.  `meta` is packed to
  // dense indices as CheckAndMallocMetaResource / CheckSubmitLimits pack it (zero-count GRES entries of a delta are dropped, as everywhere),
  // the whole batch runs on the device, and the maps of `meta` are written back: user_meta, account_meta and qos_meta hold what the
  // reference's per-job loop leaves: values subtracted or zeroed, erased nested entries erased, for a charge the created records and
  // entities.  report[j] (releases) lists per record the reference's two messages: `not_found` (:1143, :1172) and `over_free` (:1152,
  // :1196), each as "<entity type> <entity name>" with the entity type of the message ("user", "account", "qos").
  // A delta with an unknown user, account, QoS or partition is not applied (report[j].skipped; a charge of one fails the call: the
  // reference would create records under names AccountManager does not know).  A (user, account) pair that is not in
  // meta.user_accounts is the reference's "account not found in the user's account list" (:1172).
  // UserAddJob / UserReduceJob (:169, :1207) stay with the caller.  false on an engine error (no device: CNS_ERR_NO_DEVICE, several
  // devices: CNS_ERR_UNSUPPORTED, no snapshot, an all-zero delta, a charge that would pass a 32-bit count): nothing is written and
  // Ok() / LastStatus() / LastError() say why; nothing is thrown.
  struct UsageDelta {
    std::string username, account, qos;
    PartitionId partition_id;
    ResourceView resource;
    uint32_t jobs_count{0}, submit_count{0};
    int64_t time_limit{0};
    static UsageDelta Of(const std::string& username, const std::string& account, const std::string& qos, const PartitionId& partition_id) {
      UsageDelta d;
      d.username = username; d.account = account; d.qos = qos; d.partition_id = partition_id;
      return d;
    }
    // FreeMetaResource(const JobInCtld&), :243-254: {allocated_res_view, 1, IsArrayChild() ? 0 : 1, time_limit}
    static UsageDelta FreeMetaResource(const std::string& username, const std::string& account, const std::string& qos, const PartitionId& partition_id,
                                       const ResourceView& allocated_res_view, int64_t time_limit, bool is_array_child) {
      UsageDelta d = Of(username, account, qos, partition_id);
      d.resource = allocated_res_view; d.jobs_count = 1; d.submit_count = is_array_child ? 0u : 1u; d.time_limit = time_limit;
      return d;
    }
    // FreeMetaRunningResource, :256-269 (a requeue): {allocated_res_view, 1, 0, time_limit}
    static UsageDelta FreeMetaRunningResource(const std::string& username, const std::string& account, const std::string& qos, const PartitionId& partition_id,
                                              const ResourceView& allocated_res_view, int64_t time_limit) {
      return FreeMetaResource(username, account, qos, partition_id, allocated_res_view, time_limit, true);
    }
    // FreeMetaResource(const PdJobInScheduler&), :271-283: {allocated_res.View(), 1, 0, time_limit}
    static UsageDelta FreeMetaResource(const PdJobInScheduler& job, const ResourceView& allocated_res_view) {
      return FreeMetaResource(job.username, job.account, job.qos, job.partition_id, allocated_res_view, job.time_limit, true);
    }
    // FreeMetaSubmitResource, :226-241: {0, 0, count, 0}; count == 0 is no call (:228)
    static UsageDelta FreeMetaSubmitResource(const std::string& username, const std::string& account, const std::string& qos, const PartitionId& partition_id,
                                             uint32_t count) {
      UsageDelta d = Of(username, account, qos, partition_id);
      d.submit_count = count;
      return d;
    }
    // MallocMetaSubmitResource, :139-153: {0, 0, count, 0}
    static UsageDelta MallocMetaSubmitResource(const std::string& username, const std::string& account, const std::string& qos, const PartitionId& partition_id,
                                               uint32_t count) {
      return FreeMetaSubmitResource(username, account, qos, partition_id, count);
    }
    // MallocMetaResourceToRecoveredRunningJob, :155-178: {allocated_res_view, 1, IsArrayChild() ? 0 : 1, time_limit}
    static UsageDelta MallocMetaResourceToRecoveredRunningJob(const std::string& username, const std::string& account, const std::string& qos,
                                                              const PartitionId& partition_id, const ResourceView& allocated_res_view, int64_t time_limit,
                                                              bool is_array_child) {
      return FreeMetaResource(username, account, qos, partition_id, allocated_res_view, time_limit, is_array_child);
    }
  };
  struct UsageReport {
    bool skipped{false};                    // an unknown name: not applied
    uint16_t not_found_bits{0}, over_free_bits{0};
    std::vector<std::string> not_found;     // "<entity type> <entity name>", in the reference's order of records
    std::vector<std::string> over_free;
  };
  bool ReleaseMetaResources(AccountMetaSnapshot* meta, const std::vector<UsageDelta>& frees, std::vector<UsageReport>* report = nullptr,
                            cns_usage_timing* timing = nullptr);
  bool ChargeMetaResources(AccountMetaSnapshot* meta, const std::vector<UsageDelta>& charges, cns_usage_timing* timing = nullptr);

  // ---- the running set kept on the device between two cycles (include/crane_gpu_running/running.h) -------------------------
  // With resident running ON, NodeSelect(now, running_jobs, pending_jobs) does not hand the running set to the engine and ignores the
  // CONTENTS of running_jobs (a multifactor sorter still reads them, unless it borrows this object's engine and UseResidentAttrs is on): the cycle runs on the device ledger.  The caller seeds the ledger
  // once and, behind every cycle, tells it what the commit loop did:
  //   SeedRunning(running_jobs)                          the whole set, once (and again after a restart); the vector's order is the
  //                                                      ledger's order (a job whose reservation is unknown is left out, as in a cycle)
  //   AdvanceRunning(finished_job_ids, admitted)         FreeResourceFromNode for the jobs that ended (CranedMetaContainer.cpp:226-277;
  //                                                      an unknown id changes nothing, :248-253), MallocResourceFromNode for the
  //                                                      jobs of the LAST NodeSelect that the commit loop started (JobScheduler.cpp:
  //                                                      1575-1628): their placements are read on the device.  `admitted` names them
  //                                                      by pointer, in any order; a job the cycle did not start now never enters.
  // A new snapshot (SetClusterSnapshot, a craned state flip) keeps the ledger while the node count stays; the next NodeSelect rebuilds
  // the per-slot tables from it first.  Default: off — NodeSelect hands the running set in as before.  One device only.
  // A cycle with preemption (a snapshot with preempt_enabled) runs on the ledger too (include/crane_gpu_running/running_preempt.h): the
  // adapter keeps the ledger's id order from SeedRunning / AdvanceRunning, looks every row's RnJobInScheduler up by id in running_jobs
  // (a row that is not there fails the cycle) and hands qos, qos_priority and start_time in in ledger order; the preempted lists point
  // at the caller's own objects.  AdvanceRunning behind such a cycle takes `admitted` as the jobs the commit loop really started: a job
  // that preempted a running job is held back by it ("Waiting for Preemption", JobScheduler.cpp:1542-1555) and must not be named.
  void UseResidentRunning(bool on);
  bool ResidentRunning() const;
  // The attribute columns beside the ledger (include/crane_gpu_running/running_attrs.h).  SeedRunning hands start_time, qos, qos_priority,
  // partition_priority and account of every RnJobInScheduler in, AdvanceRunning those of the admitted PdJobInScheduler (its start is the
  // cycle's now).  Account names map to dense ids through a grow-only table kept across cycles: an id, once given, never moves;
  // NumAccounts() is its size.  ResidentAttrs(): resident running is on and the ledger carries the columns — then a
  // GpuMultiFactorPriority built over this object ranks from the ledger, and NodeSelect with preempt_enabled packs no per-row arrays
  // (cns_running_select_preempt_attrs; it still needs the caller's objects to resolve the preempted lists by ledger id).
  // Opt-in (UseResidentAttrs(true) before SeedRunning), because a row admitted with the columns starts at the cycle's now whatever
  // start_time the caller later writes into its own RnJobInScheduler: a caller that keeps another start there and wants TryPreempt_ to
  // see it stays on the plain calls.
  void UseResidentAttrs(bool on);
  bool ResidentAttrs() const;
  uint32_t AccountId(const std::string& account);
  uint32_t NumAccounts() const;
  cns_engine* EngineHandle() const;
  bool SeedRunning(const std::vector<std::unique_ptr<RnJobInScheduler>>& running_jobs);
  bool AdvanceRunning(const std::vector<job_id_t>& finished_job_ids, const std::vector<const PdJobInScheduler*>& admitted,
                      uint64_t* num_retired = nullptr, uint64_t* num_admitted = nullptr);
  // A running job's end time changed (include/crane_gpu_amend/running_amend.h): JobScheduler::ChangeJobTimeConstraint's SetEndTime
  // (JobScheduler.cpp:2411-2413; an array parent: one pair per running child, :2312-2321) and ResumeSuspendedJobs (:2833-2857).  Valid
  // with resident running on; (job id, new end_time) pairs in any order, ids distinct.  The ledger's end column and the per-slot
  // running tables follow on the device: no re-seed.  A job the ledger does not carry changes nothing and is not counted in
  // *num_amended.  With resident running on, QueryReservation takes its running side from the ledger (cns_resvq_set_state_resident)
  // and refreshes it behind SeedRunning, AdvanceRunning, AmendRunning and a new snapshot.
  bool AmendRunning(const std::vector<std::pair<job_id_t, TimeSec>>& new_ends, uint64_t* num_amended = nullptr);

  // ---- event-fed mirror of the running allocations -------------------------------------------------
  // Instead of re-deriving the running jobs' allocations from the vector NodeSelect is handed every cycle, the adapter
  // can be told what the meta container is told: the same calls, at the same places (JobScheduler.cpp:1590-1612 for the
  // start of a job, the job-end path for the release) —
  //   MallocResourceFromNode(craned, job, resources)   CranedMetaContainer.cpp:178-224
  //   FreeResourceFromNode(craned, job)                CranedMetaContainer.cpp:226-277
  // plus the two facts of RnJobInScheduler the meta container does not hold: the job's end time and its reservation.
  // The allocation is packed ONCE, when it is made; NodeSelect(now, pending_jobs) then runs the cycle on the mirror
  // (running jobs in ascending job id, the order of the reference's running-job map).  A new snapshot re-packs the
  // mirror (dense node indices and GRES bit positions are per snapshot).
  void MallocResourceFromNode(const CranedId& craned_id, job_id_t job_id, const ResourceV3& resources);
  void FreeResourceFromNode(const CranedId& craned_id, job_id_t job_id);
  void SetRunningJobInfo(job_id_t job_id, TimeSec end_time, const std::string& reservation = "");
  size_t MirroredRunningJobs() const;
  // how the mirror was packed so far: full walks over the job map / patches of the packed form kept from the previous cycle
  void MirrorPackCounts(size_t* full_walks, size_t* patches) const;
  // (`running_for_priority`: only read by a multifactor sorter, JobScheduler.cpp:7692-7746; not needed with BasicPriority)
  void NodeSelect(const TimeSec& now, const std::vector<std::unique_ptr<PdJobInScheduler>>& pending_jobs,
                  const std::vector<std::unique_ptr<RnJobInScheduler>>* running_for_priority = nullptr);

  // The run-limit admission of the commit loop, batched: AccountMetaContainer::CheckAndMallocMetaResource
  // (AccountMetaContainer.cpp:180-224) for every job of `pending_jobs` — in THAT order, JobScheduler.cpp:1492 — that the
  // last NodeSelect started (`reason` empty).  results[i] = "" (admitted: `meta`'s usage maps now include the job, as
  // after DoMallocResource_) or the pending reason the reference would set ("QosJobsResourceLimit", ...); jobs with a
  // reason keep it.  The NodeSelect results are read where they are, on the device (include/crane_gpu/run_limits.h).
  // GRES names / types no node of the snapshot has are dropped from limits and usage (no job can allocate them).
  void CheckAndMallocMetaResource(AccountMetaSnapshot& meta, const std::vector<std::unique_ptr<PdJobInScheduler>>& pending_jobs,
                                  std::vector<std::string>& results);

  // JobScheduler::StepScheduleThread_'s loop (JobScheduler.cpp:1992-2001) in one call: SchedulePendingSteps for every
  // job of `jobs`.  Steps that were scheduled get `scheduled`, craned_ids, allocated_res, craned_task_map and
  // task_res_map; each job's step_res_avail is updated; the first step of a job that does not fit stops that job's
  // queue.  A job's nodes are walked in the order of the snapshot (the reference walks an unordered_map).  A pass the engine refuses
  // (include/crane_gpu/steps.h, "Limits": CNS_ERR_UNSUPPORTED in LastStatus()) leaves every step pending: the caller keeps them.
  void SchedulePendingSteps(std::vector<JobStepQueue>& jobs);

  // Measurement / test hook: only the host-side packing of the running jobs (what NodeSelect does before
  // cns_set_running), with or without the per-job cache; needs no device.  Returns the number of allocation records,
  // *checksum covers every array cns_set_running would receive, *pack_ms is the packing alone.
  // ... and of the pending side: cns_job_soa packing + the write-back of (synthetic) placements into the jobs.
  void PendingCycleForBench(const std::vector<std::unique_ptr<PdJobInScheduler>>& pending_jobs, double* pack_ms,
                            double* write_back_ms, uint64_t* checksum);
  size_t PackRunningForBench(const std::vector<std::unique_ptr<RnJobInScheduler>>& running_jobs, bool use_cache,
                             uint64_t* checksum, double* pack_ms = nullptr);
  // ... the same from the event-fed mirror.  *checksum_canonical (both functions) does not depend on the order of a job's
  // per-node records (the explicit path walks an unordered_map, the mirror keeps event order).
  size_t PackMirrorForBench(uint64_t* checksum_canonical, double* pack_ms = nullptr);
  uint64_t LastRunningChecksumCanonical() const;
  // true: the running set packed last (PackRunningForBench / PackMirrorForBench / a NodeSelect) holds an allocation with a core
  // id >= 256 — such a cycle is refused with CNS_ERR_UNSUPPORTED for as long as the job runs (the bit is kept with the cached /
  // mirrored record, not with the cycle that first packed it)
  bool PackedRunningSetOverflows() const;

  // ---- placement -> wire: the protobuf encoding of what JobToD carries, written straight from the
  // packed placements of the last NodeSelect — no ResourceInNodeV3 object, no std::set, no map is built on the way.
  //   crane.grpc.ResourceInNodeV3 {cpu_ids=1 (packed), cpu_count=2, memory_bytes=3, memory_sw_bytes=4, gres=5}
  //                                                  protos/PublicDefs.proto:63-69, PublicHeader.cpp:981-998,255-266
  //   crane.grpc.JobToD {job_id=1, uid=2, res=4, partition=5, account=6, qos=7, name=9}
  //                                                  protos/PublicDefs.proto:396-409, CtldPublicDefs.cpp:537-554
  // Fields are written in field-number order, map entries in (name, type) order and slots in std::set order, i.e. what
  // protobuf's deterministic serialisation of the reference's message produces.
  struct WireBatch {
    struct Rec { uint32_t job, node, off, len; };   // job: index in the vector handed to NodeSelect's order (LastOrder())
    std::string bytes;                              // the serialised ResourceInNodeV3 messages, back to back
    std::vector<Rec> recs;                          // one per (job that starts now, allocated node), queue order
  };
  // every allocation of the jobs that start in this cycle; returns the number of records
  size_t EmitStartedResourcesWire(WireBatch* out) const;
  const std::vector<const PdJobInScheduler*>& LastOrder() const;
  // one allocation / one JobToD of a job of the last cycle (appends to *out; false: job or node not in the last cycle's result)
  bool AppendResourceInNodeV3Wire(const PdJobInScheduler& job, const CranedId& craned_id, std::string* out);
  // JobToD.array_task (field 16, ArrayTaskIdentity{array_job_id, task_id}): set by the reference for array children only
  // (GetArrayTaskIdentity(), CtldPublicDefs.cpp:547-551); pass the identity to emit it, nullptr for every other job.
  struct ArrayTaskIdentity { uint32_t array_job_id; uint32_t task_id; };
  bool AppendJobToDWire(const PdJobInScheduler& job, uint32_t uid, const std::string& name, const CranedId& craned_id,
                        std::string* out, const ArrayTaskIdentity* array_task = nullptr);
  static void ComposeJobToDWire(uint32_t job_id, uint32_t uid, const std::string& partition, const std::string& account,
                                const std::string& qos, const std::string& name, const std::string& res_wire, std::string* out,
                                const ArrayTaskIdentity* array_task = nullptr);
  // test / bench hook (no device): the wire bytes and the ResourceInNodeV3 object of one packed allocation
  void WireOfPackedForTest(int64_t cpu_raw, uint64_t mem, uint64_t mem_sw, uint64_t core_lo, uint64_t core_hi, uint64_t gres,
                           std::string* wire, ResourceInNodeV3* obj, uint64_t core_w2 = 0, uint64_t core_w3 = 0) const;
  // ... and the emission of PendingCycleForBench's synthetic placements (ms per call)
  double EmitWireForBench(size_t* records, size_t* bytes);

  // ---- test hooks (no device): the two halves of the string <-> ABI translation, checked against an independent derivation ----------
  // Copies of every array the adapter hands to cns_set_nodes ("n_*", "part_*", "layout_*"), cns_set_reservations ("v_*"),
  // cns_set_running ("r_*", after packing `running_jobs`) and cns_select ("j_*", after packing `pending_jobs` in their order; no sorter,
  // no license pre-pass), each as 64-bit words (signed values two's complement).  Needs SetClusterSnapshot first.
  void PackedArraysForTest(const std::vector<std::unique_ptr<RnJobInScheduler>>& running_jobs,
                           const std::vector<std::unique_ptr<PdJobInScheduler>>& pending_jobs,
                           std::map<std::string, std::vector<uint64_t>>* out);
  // cns_placement_soa of a cycle over `pending_jobs` (in their order), as the caller gives it
  struct PlacementsForTest {
    std::vector<int64_t> start_sec;
    std::vector<uint8_t> reason;
    std::vector<uint64_t> place_offsets;   // [J + 1]
    std::vector<uint32_t> node_idx, ntasks;
    std::vector<int64_t> cpu_raw;
    std::vector<uint64_t> mem, core_lo, core_hi, gres, core_w2, core_w3;
  };
  // The write-back of those placements into the jobs, under the current write-back mode, exactly as NodeSelect runs it; afterwards
  // they are the last cycle's placements (MaterializeAllocation, the wire emission).
  void WriteBackForTest(const std::vector<std::unique_ptr<PdJobInScheduler>>& pending_jobs, const PlacementsForTest& p);

  // ---- preemption (only when the snapshot had preempt_enabled) -------------------------------------------------------
  // m_preempting_set_ (JobScheduler.h:984) lives in the adapter across cycles; the running jobs newly put into it by the
  // last cycle are what the reference hands to EnqueuePreemptCancel (JobScheduler.cpp:6793), in that order.
  const std::vector<job_id_t>& LastPreemptCancel() const;
  const std::set<job_id_t>& PreemptingSet() const;

  bool Ok() const { return status_ == 0; }
  // wall time of the three parts of the last NodeSelect: packing the pending jobs | cns_select (H2D of the job table, the kernels, D2H
  // of the placements; the arrays live in page-locked memory of the engine, kept across cycles) | write-back into the job objects
  void LastCycleMs(double* pack_ms, double* engine_ms, double* write_back_ms) const;
  int LastStatus() const { return status_; }
  const std::string& LastError() const { return error_; }

 private:
  struct Impl;
  std::unique_ptr<Impl> impl_;
  void SelectPacked_(const TimeSec& now, const std::vector<std::unique_ptr<PdJobInScheduler>>& pending_jobs,
                     const std::vector<std::unique_ptr<RnJobInScheduler>>& running_jobs);
  bool ApplyMetaUsage_(uint32_t op, const char* who, AccountMetaSnapshot* meta, const std::vector<UsageDelta>& deltas, std::vector<UsageReport>* report,
                       cns_usage_timing* timing);
  IPrioritySorter* sorter_{nullptr};
  std::unordered_map<std::string, License> licenses_;
  uint64_t batch_{0};
  int status_{0};
  std::string error_;
};

}  // namespace crane
