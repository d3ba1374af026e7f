"""The dependency-event drain and Phase 1 of ScheduleThread_ (src/CraneCtld/JobScheduler.cpp:1353-1413) restated statement by statement,
with DependenciesInJob (CtldPublicDefs.h:454-469, CtldPublicDefs.cpp:145-160) and the array parent's gate (Array.cpp:683-699, :236-259)
as the reference writes them: a dict per job that entries are erased from, the events applied one by one in queue order.  This is the
truth the engine's cns_gate_pending is held to; it is NOT the device algorithm (no "first event wins", no compaction by scan).

Times are whole seconds; INF / -INF stand for absl::InfiniteFuture() / InfinitePast().  absl::Time + absl::Duration saturates; abseil is
not available here, so the rule of include/crane_gpu_gate/pending_gate.h is restated in `time_plus_seconds` and is the contract."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Optional

import numpy as np

INF = (1 << 63) - 1       # absl::InfiniteFuture()
NINF = -(1 << 63)         # absl::InfinitePast()

(OK, OK_ARRAY_PARENT, HELD, BEGIN_TIME, DEPENDENCY, DEPENDENCY_NEVER, ARRAY_NO_META, ARRAY_COMPLETE, ARRAY_CANCELLED, ARRAY_DEADLINE,
 ARRAY_NO_NEXT, ARRAY_TASK_LIMIT) = range(12)
# what the reference leaves in job->pending_reason
REASON = {OK: "", OK_ARRAY_PARENT: "", HELD: "Held", BEGIN_TIME: "BeginTime", DEPENDENCY: "Dependency",
          DEPENDENCY_NEVER: "DependencyNeverSatisfied", ARRAY_NO_META: "", ARRAY_COMPLETE: "ArrayMaterializationComplete",
          ARRAY_CANCELLED: "Cancelled", ARRAY_DEADLINE: "Deadline", ARRAY_NO_NEXT: "", ARRAY_TASK_LIMIT: "ArrayTaskLimit"}
CODE_OF_REASON = {"Held": HELD, "BeginTime": BEGIN_TIME, "Dependency": DEPENDENCY, "DependencyNeverSatisfied": DEPENDENCY_NEVER,
                  "ArrayMaterializationComplete": ARRAY_COMPLETE, "Cancelled": ARRAY_CANCELLED, "Deadline": ARRAY_DEADLINE,
                  "ArrayTaskLimit": ARRAY_TASK_LIMIT}


def time_plus_seconds(t: int, seconds: int) -> int:
    """absl::Time + absl::Seconds(uint64): an infinite time stays what it is; a delay >= 2^63 does not fit the duration's signed seconds
    and is +infinity; else the sum saturates at InfiniteFuture."""
    if t in (INF, NINF):
        return t
    if seconds >= 1 << 63:
        return INF
    return min(t + seconds, INF)


@dataclass
class Dependencies:
    """DependenciesInJob, CtldPublicDefs.h:454-469"""
    deps: dict = field(default_factory=dict)   # dependee job id -> (type, delay seconds); the type is not modelled
    is_or: bool = False
    ready_time: int = NINF                     # :458

    def is_met(self, now: int) -> bool:        # :460-462
        return (self.is_or or len(self.deps) == 0) and self.ready_time <= now

    def is_failed(self) -> bool:               # :464-466
        return self.ready_time >= INF and ((not self.is_or) or len(self.deps) == 0)

    def update(self, job_id: int, event_time: int) -> bool:   # CtldPublicDefs.cpp:145-160; -> whether an entry was found
        if job_id not in self.deps:                            # :146-150
            return False
        delay_seconds = self.deps[job_id]                      # :151
        dep_ready_time = time_plus_seconds(event_time, delay_seconds)   # :153
        if self.is_or:                                         # :154
            self.ready_time = min(self.ready_time, dep_ready_time)
        else:
            self.ready_time = max(self.ready_time, dep_ready_time)     # :157
        del self.deps[job_id]                                  # :159
        return True


@dataclass
class ArrayParent:
    """What PrepareParentForMaterialization and SpawnBlockReason read (Array.cpp:683-699, :236-259)."""
    has_meta: bool = True            # FindMeta_(parent.JobId()) != nullptr
    has_parent: bool = True          # parent_job_ != nullptr
    complete: bool = False           # ArrayMaterializationComplete()
    cancel: bool = False             # CancelRequested()
    deadline: int = INF              # parent_job_->deadline_time
    has_next: bool = True            # NextMaterializableTaskId().has_value()
    running: int = 0                 # RunningChildCount()
    run_limit: int = 1 << 40         # EffectiveRunLimit(array_spec)

    def spawn_block_reason(self, now: int) -> Optional[str]:   # Array.cpp:236-259; None = std::nullopt
        if not self.has_parent:                                # :237
            return ""
        if self.complete:                                      # :240
            return "ArrayMaterializationComplete"
        if self.cancel:                                        # :243
            return "Cancelled"
        if self.deadline <= now:                               # :246
            return "Deadline"
        if not self.has_next:                                  # :249
            return ""
        if self.running >= self.run_limit:                     # :255
            return "ArrayTaskLimit"
        return None

    def prepare(self, now: int):
        """PrepareParentForMaterialization, Array.cpp:683-699 -> (can_materialize, pending_reason, the code of include/.../pending_gate.h)"""
        if not self.has_meta:                                  # :687-690
            return False, "", ARRAY_NO_META
        reason = self.spawn_block_reason(now)                  # :692
        if reason is None:                                     # :693-694
            return True, "", OK_ARRAY_PARENT
        if reason == "":                                       # the two "" returns: which one, for the code
            return False, "", ARRAY_NO_META if not self.has_parent else ARRAY_NO_NEXT
        return False, reason, CODE_OF_REASON[reason]           # :696


@dataclass
class Job:
    """The fields of JobInCtld that :1377-1413 read."""
    job_id: int
    held: bool = False
    begin_time: int = NINF
    dependencies: Dependencies = field(default_factory=Dependencies)
    array: Optional[ArrayParent] = None        # IsArrayParent()


@dataclass
class Result:
    code: np.ndarray          # [J] in ascending job id
    pending: np.ndarray       # rows of pending_jobs, in the order of the emplace_back calls
    ready_sec: np.ndarray     # [J] ready_time after the events
    counts: np.ndarray        # [16]
    ev_stats: np.ndarray      # [3] applied, no such pending job, no such dependency
    reasons: list = field(default_factory=list)   # pending_reason per row
    materializes: list = field(default_factory=list)


def gate(now: int, jobs: list, events: list) -> Result:
    """jobs: [Job], mutated as the reference mutates its JobInCtld (deps erased, ready_time folded); events: [(dependent, dependee,
    event_time)] in queue order."""
    pending_job_map = {j.job_id: j for j in sorted(jobs, key=lambda j: j.job_id)}   # m_pending_job_map_: a btree_map, ascending ids
    assert len(pending_job_map) == len(jobs), "job ids are the keys of a map"
    ev_stats = [0, 0, 0]
    for dependent, dependee, event_time in events:             # :1361
        job = pending_job_map.get(dependent)                   # :1362
        if job is not None:                                    # :1363
            found = job.dependencies.update(dependee, event_time)   # :1364 UpdateDependency
            ev_stats[0 if found else 2] += 1
            continue                                           # :1366
        ev_stats[1] += 1                                       # :1369-1370: nobody to update
    code, pending, reasons, mat = [], [], [], []
    for row, job in enumerate(pending_job_map.values()):       # :1377
        if job.held:                                           # :1380
            code.append(HELD); reasons.append("Held"); continue
        if job.begin_time > now:                               # :1384
            code.append(BEGIN_TIME); reasons.append("BeginTime"); continue
        if not job.dependencies.is_met(now):                   # :1388
            if job.dependencies.is_failed():                   # :1389
                code.append(DEPENDENCY_NEVER); reasons.append("DependencyNeverSatisfied")
            else:
                code.append(DEPENDENCY); reasons.append("Dependency")   # :1392
            continue
        if job.array is not None:                              # :1397
            can, reason, c = job.array.prepare(now)            # :1398-1399
            if not can:                                        # :1400
                code.append(c); reasons.append(reason); continue
            code.append(OK_ARRAY_PARENT); reasons.append("")   # :1404
            pending.append(row); mat.append(True)              # :1405-1407
            continue
        code.append(OK); reasons.append("")
        pending.append(row); mat.append(False)                 # :1411-1412
    counts = np.zeros(16, np.uint64)
    for c in code:
        counts[c] += 1
    ready = np.asarray([j.dependencies.ready_time for j in pending_job_map.values()], np.int64)
    return Result(np.asarray(code, np.uint8), np.asarray(pending, np.uint32), ready, counts, np.asarray(ev_stats, np.uint64), reasons, mat)
