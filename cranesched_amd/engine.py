"""ctypes binding of the engine's C ABI (include/crane_gpu/node_select.h).

`GpuNodeSelector` is the Python mirror of the reference's `SchedulerAlgo` plugin surface
(src/CraneCtld/JobScheduler.h:233-263): one object per controller, `node_select(now, running,
pending)` once per scheduling cycle.  The work happens in the HIP shared library; this module
fails loudly if that library is missing or no MI355X is visible — there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
# torch first: its wheel bundles its own HIP/HSA runtime (SONAME libamdhip64.so.7).  Loading it before
# the engine makes the dynamic loader hand the SAME runtime to libcrane_gpu_nodeselect.so; two HIP
# runtimes in one process leave the second one without devices (hipGetDeviceCount -> "no ROCm-capable
# device").  torch is plumbing here (device memory for RCCL, torch.distributed), never on the hot path.
import torch  # noqa: F401  (must precede the CDLL below)

from . import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CNS_ENGINE_LIB") or os.path.join(_HERE, "libcrane_gpu_nodeselect.so")
_LIB = None

# every symbol include/crane_gpu/node_select.h declares
ABI_SYMBOLS = ("cns_abi_version", "cns_last_error", "cns_create", "cns_destroy", "cns_set_nodes",
               "cns_set_reservations", "cns_set_running", "cns_set_host_threads", "cns_select", "cns_upload_jobs", "cns_run_resident", "cns_download",
               "cns_device_results", "cns_host_alloc", "cns_host_free", "cns_get_timing", "cns_debug_get_costs", "cns_debug_get_timeline", "cns_debug_get_timeline_cores",
               "cns_debug_last_kernel", "cns_debug_get_prof", "cns_debug_engine_partitions", "cns_select_shape", "cns_serial_shape",
               # several devices (csrc/group_host.inc)
               "cns_get_partition_status",
               "cns_results_layout", "cns_comm_unique_id", "cns_comm_init_rank", "cns_comm_destroy", "cns_allgather_results",
               "cns_download_gathered", "cns_gather_timing", "cns_group_create", "cns_group_destroy", "cns_group_last_error",
               "cns_group_size", "cns_group_handle", "cns_group_set_nodes", "cns_group_set_reservations", "cns_group_set_running",
               "cns_group_select", "cns_group_get_info", "cns_group_device_of_partition", "cns_group_get_partition_status")
# ... and include/crane_gpu/priority.h
PRIORITY_ABI_SYMBOLS = ("cns_priority_order", "cns_priority_timing")
# ... and include/crane_gpu/run_limits.h
# ... and include/crane_gpu/steps.h
STEPS_ABI_SYMBOLS = ("cns_schedule_steps",)
# ... and include/crane_gpu/preempt.h
PREEMPT_ABI_SYMBOLS = ("cns_select_preempt", "cns_preempt_shape")
# ... and include/crane_gpu_probe/probe.h
PROBE_ABI_SYMBOLS = ("cns_probe", "cns_probe_upload", "cns_probe_run_resident", "cns_probe_download", "cns_probe_shape")
PROBE_DEBUG_ABI_SYMBOLS = ("cns_debug_get_probe_plan", "cns_debug_get_dips")
# ... and include/crane_gpu_resv/resv_probe.h
RESVQ_ABI_SYMBOLS = ("cns_resvq_set_state", "cns_resvq_run", "cns_resvq_shape")
# ... and include/crane_gpu_valid/validity.h
VALID_ABI_SYMBOLS = ("cns_validate_jobs", "cns_validate_shape")
# ... and include/crane_gpu_commit/commit_check.h
COMMIT_ABI_SYMBOLS = ("cns_commit_check", "cns_commit_shape")
# ... and include/crane_gpu_submit/submit_limits.h
SUBMIT_ABI_SYMBOLS = ("cns_set_submit_limits", "cns_check_submissions", "cns_get_submit_usage", "cns_get_submit_timing", "cns_submit_shape")
# ... and include/crane_gpu_usage/usage.h
USAGE_ABI_SYMBOLS = ("cns_usage_set_tables", "cns_usage_apply", "cns_usage_get_tables", "cns_usage_get_timing", "cns_usage_shape")
# ... and include/crane_gpu_gate/pending_gate.h
GATE_ABI_SYMBOLS = ("cns_gate_pending", "cns_gate_shape")
# ... and include/crane_gpu_running/running.h
RUNNING_ABI_SYMBOLS = ("cns_running_seed", "cns_running_advance", "cns_running_get", "cns_running_get_timing", "cns_running_shape")
# ... and include/crane_gpu_running/running_preempt.h
RUNNING_PREEMPT_ABI_SYMBOLS = ("cns_running_select_preempt", "cns_debug_get_preempt_index", "cns_running_preempt_get_timing")
# ... and include/crane_gpu_running/running_attrs.h
RUNNING_ATTRS_ABI_SYMBOLS = ("cns_running_seed_attrs", "cns_running_advance_attrs", "cns_running_get_attrs", "cns_priority_order_resident",
                             "cns_running_select_preempt_attrs")
# ... and include/crane_gpu_amend/running_amend.h
RUNNING_AMEND_ABI_SYMBOLS = ("cns_running_amend_ends", "cns_running_amend_get_timing", "cns_resvq_set_state_resident")
LIMITS_ABI_SYMBOLS = ("cns_set_run_limits", "cns_apply_run_limits", "cns_upload_limit_jobs", "cns_run_limits_resident",
                      "cns_download_limits", "cns_get_limit_timing", "cns_get_usage", "cns_limits_shape")


class EngineError(RuntimeError):
    def __init__(self, status: int, msg: str):
        super().__init__(f"{abi.STATUS_STR.get(status, status)}: {msg}")
        self.status = status


def lib():
    """Load the HIP engine. Raises if it has not been built (python -c 'import __graft_entry__ as g; g.build()')."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise FileNotFoundError(
                f"{LIB_PATH} is missing: the HIP engine is not built and there is no CPU fallback. "
                "Run `python -c 'import __graft_entry__ as g; g.build()'`.")
        L = C.CDLL(LIB_PATH)
        L.cns_last_error.restype = C.c_char_p
        L.cns_last_error.argtypes = [C.c_void_p]
        L.cns_destroy.restype = None
        L.cns_destroy.argtypes = [C.c_void_p]
        L.cns_debug_last_kernel.restype = C.c_char_p
        L.cns_debug_last_kernel.argtypes = [C.c_void_p]
        if not hasattr(L, "cns_group_create"):   # (an older build of the engine, loaded through CNS_ENGINE_LIB for an A/B run: tools/var_bench.py)
            _LIB = L
            return _LIB
        L.cns_group_last_error.restype = C.c_char_p
        L.cns_group_last_error.argtypes = [C.c_void_p]
        L.cns_group_destroy.restype = None
        L.cns_group_destroy.argtypes = [C.c_void_p]
        L.cns_group_handle.restype = C.c_void_p
        L.cns_group_handle.argtypes = [C.c_void_p, C.c_uint32]
        L.cns_group_size.restype = C.c_uint32
        L.cns_group_size.argtypes = [C.c_void_p]
        L.cns_group_device_of_partition.restype = C.c_uint32
        L.cns_group_device_of_partition.argtypes = [C.c_void_p, C.c_uint32]
        _LIB = L
    return _LIB


def resvq_shape() -> "abi.ResvqShape":
    """cns_resvq_shape: the constants the reservation what-ifs' kernels are compiled with.  Needs no handle and no GPU."""
    v = [C.c_uint32(0) for _ in abi.ResvqShape._fields]
    status = lib().cns_resvq_shape(*[C.byref(x) for x in v])
    if status != 0:
        raise EngineError(status, "cns_resvq_shape")
    return abi.ResvqShape(*[x.value for x in v])


def preempt_shape() -> "abi.PreemptShape":
    """cns_preempt_shape: the sizes the device form of TryPreempt_ is compiled with.  Needs no handle and no GPU."""
    v = [C.c_uint32(0) for _ in abi.PreemptShape._fields]
    status = lib().cns_preempt_shape(*[C.byref(x) for x in v])
    if status != 0:
        raise EngineError(status, "cns_preempt_shape")
    return abi.PreemptShape(*[x.value for x in v])


def select_shape() -> "abi.SelectShape":
    """cns_select_shape: the constants at which the selection kernels change path, as this build has them.  Needs no handle and no GPU."""
    s = abi.CnsSelectShapeInfo()
    status = lib().cns_select_shape(C.byref(s))
    if status != 0:
        raise EngineError(status, "cns_select_shape")
    tile = lambda t: abi.TileShape(int(t.lanes), tuple(int(w) for w in t.widths[:t.num_widths]))
    scalars = [int(getattr(s, f)) for f in abi.SelectShape._fields[:-3]]
    return abi.SelectShape(*scalars, tile(s.select), tile(s.pipe), tuple((int(s.wide_waves[b]), tile(s.wide[b])) for b in range(4)))


def serial_shape() -> "abi.SerialShape":
    """cns_serial_shape: the loop shapes of the serial protocol (k_mem, k_giant), as this build has them.  Needs no handle and no GPU."""
    s = abi.CnsSerialShapeInfo()
    status = lib().cns_serial_shape(C.byref(s))
    if status != 0:
        raise EngineError(status, "cns_serial_shape")
    return abi.SerialShape(*[int(getattr(s, f)) for f in abi.SerialShape._fields])


def probe_shape() -> "abi.ProbeShape":
    """cns_probe_shape: the constants at which k_probe changes path, as this build has them.  Needs no handle and no GPU."""
    s = abi.CnsProbeShapeInfo()
    status = lib().cns_probe_shape(C.byref(s))
    if status != 0:
        raise EngineError(status, "cns_probe_shape")
    return abi.ProbeShape(*[int(getattr(s, f)) for f in abi.ProbeShape._fields])


class GpuNodeSelector:
    """One engine handle on one MI355X (one process per GPU)."""

    def __init__(self, device: int = 0, scheduled_batch_size: int = 0, max_job_num_per_node: int = 0,
                 max_time_window_sec: int = 0, kernel_pin: int = 0):
        """kernel_pin: cns_kernel_pin — 0 the engine chooses per launch; 1 k_select, 2 k_pipe (one workgroup per partition: for a controller
        that shares its GPU with other processes, since k_wide's workgroups must all be resident at once)."""
        self._L = lib()
        self._h = C.c_void_p()
        cfg = abi.CnsConfig(abi.CNS_ABI_VERSION, device, scheduled_batch_size, max_job_num_per_node, kernel_pin,
                            max_time_window_sec)
        rc = self._L.cns_create(C.byref(cfg), C.byref(self._h))
        if rc != 0:
            msg = self._L.cns_last_error(None)
            self._h = C.c_void_p()
            raise EngineError(rc, msg.decode() if msg else "")
        self._cluster = None
        self._jobs = None
        self._pinned = {}   # address -> array over a cns_host_alloc buffer (cns_destroy releases the memory: do not touch them after close())

    # -- plumbing -----------------------------------------------------------------------------
    def _check(self, rc: int):
        if rc != 0:
            msg = self._L.cns_last_error(self._h)
            raise EngineError(rc, msg.decode() if msg else "")

    # -- MultiFactorPriority (include/crane_gpu/priority.h) ---------------------------------------
    def priority_order(self, now: int, cfg, num_accounts: int, pending, running=None, limit: int | None = None):
        """IPrioritySorter::GetOrderedJobPtrVec for PriorityType multifactor (JobScheduler.cpp:7606-7631).
        Returns (order, priority, num_ordered): order[i] = input index of the i-th job by descending priority
        (ties: ascending index), priority[j] per input job, num_ordered = min(J, limit)."""
        J = pending.num_jobs
        order = np.empty(max(J, 1), np.uint32)
        prio = np.empty(max(J, 1), np.float64)
        nord = C.c_uint64(0)
        c_cfg, c_pd = cfg.to_c(), pending.to_c()
        c_rn = running.to_c() if running is not None else None
        self._check(self._L.cns_priority_order(
            self._h, C.c_int64(now), C.byref(c_cfg), C.c_uint32(num_accounts), C.byref(c_pd),
            C.byref(c_rn) if c_rn is not None else None, C.c_uint64(J if limit is None else limit),
            order.ctypes.data_as(C.c_void_p), prio.ctypes.data_as(C.c_void_p), C.byref(nord)))
        return order[:J], prio[:J], int(nord.value)

    def priority_timing(self):
        ms, nb = C.c_double(0), C.c_uint64(0)
        self._check(self._L.cns_priority_timing(self._h, C.byref(ms), C.byref(nb)))
        return {"kernels_ms": ms.value, "algorithmic_bytes": int(nb.value)}

    # -- run-limit admission (include/crane_gpu/run_limits.h) --------------------------------------
    def set_run_limits(self, tables):
        """Limits + usage at the start of the commit loop (AccountMetaContainer state); after set_nodes."""
        t = tables.to_c()
        self._check(self._L.cns_set_run_limits(self._h, C.byref(t)))
        self._lim_tables = tables

    def apply_run_limits(self, jobs):
        """CheckAndMallocMetaResource over the last node_select's results, in the order of `jobs`
        (JobScheduler.cpp:1492-1573).  Returns (limit_reason[J] u8, num_admitted)."""
        self.upload_limit_jobs(jobs)
        self.run_limits_resident()
        return self.download_limits()

    def upload_limit_jobs(self, jobs):
        cj = jobs.to_c()
        self._check(self._L.cns_upload_limit_jobs(self._h, C.byref(cj)))
        self._lim_jobs = jobs

    def run_limits_resident(self):
        self._check(self._L.cns_run_limits_resident(self._h))

    def download_limits(self):
        J = self._lim_jobs.num_jobs
        out = np.zeros(max(J, 1), np.uint8)
        adm = C.c_uint64(0)
        self._check(self._L.cns_download_limits(self._h, out.ctypes.data_as(C.c_void_p), C.byref(adm)))
        return out[:J], int(adm.value)

    def limit_timing(self) -> dict:
        from . import limits as lm
        t = lm.CnsLimitTiming()
        self._check(self._L.cns_get_limit_timing(self._h, C.byref(t)))
        return {f: getattr(t, f) for f, _ in lm.CnsLimitTiming._fields_}

    def limits_shape(self):
        """(min_item_chunk, num_chunks, batch, carry_row_chunks, max_rounds, scan_jobs): where the run-limit kernels' paths change."""
        v = [C.c_uint32(0) for _ in range(6)]
        self._check(self._L.cns_limits_shape(*[C.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def usage(self):
        """Usage tables after the last admission (what DoMallocResource_ left)."""
        u = self._lim_tables.empty_usage()
        self._check(self._L.cns_get_usage(self._h, *u.pointers()))
        return u

    # -- step scheduler (include/crane_gpu/steps.h) ------------------------------------------------
    def schedule_steps(self, step_jobs, steps):
        """JobInCtld::SchedulePendingSteps for every job with pending steps (CtldPublicDefs.cpp:2038-2159); after
        set_nodes (GRES layout).  Returns (StepResults, kernel_ms)."""
        from . import steps as st
        out = st.StepResults(step_jobs, steps)
        cj, cs, co = step_jobs.to_c(), steps.to_c(), out.to_c()
        ms = C.c_double(0)
        self._check(self._L.cns_schedule_steps(self._h, C.byref(cj), C.byref(cs), C.byref(co), C.byref(ms)))
        return out, ms.value

    def close(self):
        if self._h:
            self._L.cns_destroy(self._h)
            self._h = C.c_void_p()
            self._pinned = {}   # (cns_destroy released them: arrays handed out by pinned() are dead from here on)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- per-cycle snapshot -----------------------------------------------------------------------
    def set_nodes(self, cluster: abi.Cluster):
        c = cluster.to_c()
        self._check(self._L.cns_set_nodes(self._h, C.byref(c)))
        self._cluster = cluster

    def partition_status(self) -> np.ndarray:
        """[P] cns_partition_status of the snapshot: 0 served; else the partition's group lies outside the engine's limits (its jobs come
        back with REASON_ENGINE_REFUSED and belong to the caller's CPU scheduler; every other partition is served)."""
        out = np.zeros(max(self._cluster.num_partitions, 1), np.uint8)
        self._check(self._L.cns_get_partition_status(self._h, out.ctypes.data_as(C.c_void_p), C.c_uint32(len(out))))
        return out[:self._cluster.num_partitions]

    def set_reservations(self, reservations: abi.Reservations | None):
        """Reservations of the cycle (JobScheduler.cpp:6619-6679): after set_nodes, before set_running."""
        if reservations is None:
            self._check(self._L.cns_set_reservations(self._h, None))
        else:
            r = reservations.to_c()
            self._check(self._L.cns_set_reservations(self._h, C.byref(r)))

    def set_running(self, running: abi.Running | None):
        if running is None:
            self._check(self._L.cns_set_running(self._h, None))
        else:
            r = running.to_c()
            self._check(self._L.cns_set_running(self._h, C.byref(r)))

    def set_host_threads(self, n: int):
        """Host threads of the engine's own pass over the queue inside cns_select / cns_upload_jobs (0: CNS_HOST_THREADS, else up to 16)."""
        self._check(self._L.cns_set_host_threads(self._h, C.c_uint32(n)))

    # -- NodeSelect --------------------------------------------------------------------------------
    def node_select(self, now: int, jobs: abi.Jobs, out: "abi.Placements | None" = None) -> abi.Placements:
        """SchedulerAlgo::NodeSelect(now, running_jobs, pending_jobs) in one call (`out`: result arrays to reuse)."""
        if out is None:
            out = abi.Placements(jobs.num_jobs, jobs.total_places())
        assert out.num_jobs == jobs.num_jobs and out.capacity >= jobs.total_places()
        cj, co = jobs.to_c(), out.to_c()
        self._check(self._L.cns_select(self._h, C.c_int64(now), C.byref(cj), C.byref(co)))
        self._jobs = jobs
        return out

    # page-locked host buffers (cns_host_alloc): the caller's job table and result arrays at full PCIe rate
    def pinned(self, n: int, dtype, fill=None) -> np.ndarray:
        """A numpy array of n elements in page-locked host memory of this handle.  It lives until free_pinned(a) or close();
        after close() the memory is gone and the array must not be touched."""
        dt = np.dtype(dtype)
        p = C.c_void_p()
        self._check(self._L.cns_host_alloc(self._h, C.c_uint64(max(n, 1) * dt.itemsize), C.byref(p)))
        a = np.frombuffer((C.c_char * (max(n, 1) * dt.itemsize)).from_address(p.value), dtype=dt)
        self._pinned[p.value] = a
        if fill is not None:
            a[:] = fill
        return a

    def free_pinned(self, a: np.ndarray):
        """Gives a buffer of pinned() (or any view of it) back (cns_host_free)."""
        base = a
        while isinstance(base.base, np.ndarray):
            base = base.base
        ptr = base.ctypes.data
        if ptr not in self._pinned:
            raise EngineError(-1, "free_pinned: not a buffer of pinned() on this handle")
        del self._pinned[ptr]
        self._check(self._L.cns_host_free(self._h, C.c_void_p(ptr)))

    def pinned_jobs(self, jobs: abi.Jobs, into: "abi.Jobs | None" = None) -> abi.Jobs:
        """The same job table with every array in page-locked memory (what an adapter that packs into such buffers hands over).
        Every call WITHOUT `into` allocates a fresh set of buffers: call it once and refill per cycle with
        `pj = eng.pinned_jobs(jobs, into=pj)` — arrays of `into` whose size still fits are overwritten in place, the others are
        freed and allocated anew; free_pinned_jobs(pj) gives a set back."""
        import dataclasses
        kw = {}
        for f in dataclasses.fields(jobs):
            v = getattr(jobs, f.name)
            old = getattr(into, f.name) if into is not None else None
            if v is None:
                if old is not None:
                    self.free_pinned(old)
                kw[f.name] = None
                continue
            if old is not None and old.dtype == v.dtype and old.size == v.size:
                old.reshape(-1)[:] = v.reshape(-1)
                kw[f.name] = old.reshape(v.shape)
                continue
            if old is not None:
                self.free_pinned(old)
            a = self.pinned(v.size, v.dtype)
            a[:v.size] = v.reshape(-1)
            kw[f.name] = a[:v.size].reshape(v.shape)
        return abi.Jobs(**kw)

    def free_pinned_jobs(self, pj: abi.Jobs):
        import dataclasses
        for f in dataclasses.fields(pj):
            v = getattr(pj, f.name)
            if v is not None:
                self.free_pinned(v)

    def pinned_placements(self, jobs: abi.Jobs) -> abi.Placements:
        """Result arrays in page-locked memory, to be reused across cycles: node_select(now, jobs, out=...)."""
        return abi.Placements(jobs.num_jobs, jobs.total_places(), alloc=self.pinned)

    # split form: inputs resident in HBM before the timed region (bench.py)
    def node_select_preempt(self, now: int, jobs: abi.Jobs, preempt: "abi.Preempt"):
        """NodeSelect with preemption (include/crane_gpu/preempt.h): TryPreempt_ between the res_total selection and the
        backfill; -> (Placements, PreemptOut).  The running set must have been handed in with set_running."""
        out = abi.Placements(jobs.num_jobs, jobs.total_places())
        pout = abi.PreemptOut(jobs.num_jobs, len(preempt.rn_job_id))
        cj, co, cp, cpo = jobs.to_c(), out.to_c(), preempt.to_c(), pout.to_c()
        self._check(self._L.cns_select_preempt(self._h, C.c_int64(now), C.byref(cj), C.byref(cp), C.byref(co), C.byref(cpo)))
        self._jobs = jobs
        return out, pout

    def upload_jobs(self, jobs: abi.Jobs):
        cj = jobs.to_c()
        self._check(self._L.cns_upload_jobs(self._h, C.byref(cj)))
        self._jobs = jobs

    def run_resident(self, now: int):
        self._check(self._L.cns_run_resident(self._h, C.c_int64(now)))

    def download(self) -> abi.Placements:
        out = abi.Placements(self._jobs.num_jobs, self._jobs.total_places())
        co = out.to_c()
        self._check(self._L.cns_download(self._h, C.byref(co)))
        return out

    # -- what-if probes against the final state of the last cycle (include/crane_gpu_probe/probe.h) ------------------------
    def probe(self, probes: abi.Jobs) -> abi.Placements:
        """When and where would each of `probes` run if it were submitted now?  Per probe what the cycle would have written for it
        behind the last job its ordered loop took, at the cycle's `now`; nothing is committed.  After a successful node_select /
        run_resident only (EngineError CNS_ERR_STATE otherwise; CNS_ERR_UNSUPPORTED after a cycle with preemption)."""
        out = abi.Placements(probes.num_jobs, probes.total_places())
        cj, co = probes.to_c(), out.to_c()
        ms = C.c_double(0)
        self._check(self._L.cns_probe(self._h, C.byref(cj), C.byref(co), C.byref(ms)))
        self._probe_ms = ms.value
        return out

    # split form: probes resident in HBM before the timed region (tools/probe_bench.py)
    def probe_upload(self, probes: abi.Jobs):
        cj = probes.to_c()
        self._check(self._L.cns_probe_upload(self._h, C.byref(cj)))
        self._probes = probes

    def probe_run_resident(self) -> float:
        """Answers the uploaded probes (again); -> HIP-event time of k_probe in ms."""
        ms = C.c_double(0)
        self._check(self._L.cns_probe_run_resident(self._h, C.byref(ms)))
        self._probe_ms = ms.value
        return ms.value

    def probe_download(self) -> abi.Placements:
        out = abi.Placements(self._probes.num_jobs, self._probes.total_places())
        co = out.to_c()
        self._check(self._L.cns_probe_download(self._h, C.byref(co)))
        return out

    def probe_timing(self) -> dict:
        """HIP-event time of the last k_probe launch of this object."""
        return {"kernel_ms": getattr(self, "_probe_ms", 0.0)}

    def probe_plan(self) -> tuple:
        """cns_debug_get_probe_plan: (workgroups, heap entries per workgroup) of the last probe_run_resident / probe."""
        g, st = C.c_uint64(0), C.c_uint32(0)
        self._check(self._L.cns_debug_get_probe_plan(self._h, C.byref(g), C.byref(st)))
        return int(g.value), int(st.value)

    def dips(self) -> dict:
        """cns_debug_get_dips: the dip the last cycle left at every (partition, node) slot, in the order of costs()."""
        n = len(self._cluster.part_nodes)
        t, cm, g = (np.zeros(n, np.uint32) for _ in range(3))
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        self._check(self._L.cns_debug_get_dips(self._h, p(t), p(cm), p(g)))
        return {"t": t, "cpus": cm >> 16, "gib": cm & 0xFFFF, "gres": g}

    # -- reservation what-ifs (include/crane_gpu_resv/resv_probe.h) --------------------------------------------------------
    def set_resv_query_state(self, running: "abi.Running | None", reservations: "abi.Reservations | None"):
        """Per-node tables for query_reservations: the latest end of the running allocations on every node and the (start, end) of
        every reservation that lists it.  After set_nodes; independent of the cycle's set_running / set_reservations."""
        rn = running.to_c() if running is not None else None
        rv = reservations.to_c() if reservations is not None else None
        self._check(self._L.cns_resvq_set_state(self._h, C.byref(rn) if rn is not None else None, C.byref(rv) if rv is not None else None))

    def set_resv_query_state_resident(self, reservations: "abi.Reservations | None"):
        """set_resv_query_state with the running side taken from the device ledger where it is (running_amend.h).  The tables do not
        follow later amends or advances: set them again."""
        rv = reservations.to_c() if reservations is not None else None
        self._check(self._L.cns_resvq_set_state_resident(self._h, C.byref(rv) if rv is not None else None))

    def query_reservations(self, now: int, queries: "abi.ResvQueries", out: "abi.ResvAnswers | None" = None) -> dict:
        """JobScheduler::CreateResv_'s node walk (JobScheduler.cpp:4383-4419) for every query at once, at its start or at the earliest
        start that fits; nothing is created.  -> {status, start_sec, num_free, code, chosen_offsets, chosen_nodes} as numpy arrays."""
        if out is None:
            out = abi.ResvAnswers(queries)
        cq, co = queries.to_c(), out.to_c()
        ms = C.c_double(0)
        self._check(self._L.cns_resvq_run(self._h, C.c_int64(now), C.byref(cq), C.byref(co), C.byref(ms)))
        self._resvq_ms = ms.value
        return out.trimmed()

    def resvq_shape(self) -> "abi.ResvqShape":
        """(pick_block, pick_grid, sort_tile, scan_span) of the reservation what-ifs' kernels: where their paths change."""
        return resvq_shape()

    def preempt_shape(self) -> "abi.PreemptShape":
        """(sort_lanes, rank_sort_max, compact_records, cache_nodes, pool_nodes) of TryPreempt_ on the device: where its paths change."""
        return preempt_shape()

    def resv_query_timing(self) -> dict:
        """HIP-event time of the kernels of the last query_reservations of this object."""
        return {"kernel_ms": getattr(self, "_resvq_ms", 0.0)}

    # -- validity of a batch of submissions (include/crane_gpu_valid/validity.h) -------------------------------------------
    def validate_jobs(self, jobs: "abi.Jobs", out=None):
        """JobScheduler::CheckJobValidity's partition checks (JobScheduler.cpp:7262-7374) for every job at once: can the job EVER run in
        its partition.  -> (code, eligible): abi.VALID_* per job, and the number of nodes of its partition that pass the walk's test.
        out: (code uint8 [J], eligible uint32 [J]) to write into, else fresh arrays."""
        j = jobs.num_jobs
        code, elig = out if out is not None else (np.zeros(max(j, 1), np.uint8), np.zeros(max(j, 1), np.uint32))
        cj = jobs.to_c()
        co = abi.CnsValidityOut(abi._ptr(code), abi._ptr(elig))
        ms = C.c_double(0)
        self._check(self._L.cns_validate_jobs(self._h, C.byref(cj), C.byref(co), C.byref(ms)))
        self._valid_ms = ms.value
        return code[:j], elig[:j]

    def validate_shape(self):
        """(node_tile, job_chunk) of the walk kernel: where its paths change."""
        a, b = C.c_uint32(0), C.c_uint32(0)
        self._check(self._L.cns_validate_shape(C.byref(a), C.byref(b)))
        return a.value, b.value

    def validity_timing(self) -> dict:
        """HIP-event time of the walk kernel of the last validate_jobs of this object."""
        return {"kernel_ms": getattr(self, "_valid_ms", 0.0)}

    # -- the commit loop's checks behind a cycle (include/crane_gpu_commit/commit_check.h) -----------------------------------
    def commit_check(self, events: "abi.CommitEvents | None", jobs: "abi.CommitJobs"):
        """The resource-reduce and preempted-still-alive checks of the commit loop (JobScheduler.cpp:1464-1555) for every job of the last
        cycle at once, on the cycle's results where they are on the device.  -> (code, counts): abi.COMMIT_* per job (the first failing
        check in the reference's order) and the number of jobs per code [8].  A code other than COMMIT_OK is a `skip` of
        apply_run_limits.  After a successful node_select / node_select_preempt / run_resident only."""
        j = jobs.num_jobs
        code, counts = np.zeros(max(j, 1), np.uint8), np.zeros(8, np.uint64)
        ce = events.to_c() if events is not None else None
        cj = jobs.to_c()
        co = abi.CnsCommitOut(abi._ptr(code), abi._ptr(counts))
        ms = C.c_double(0)
        self._check(self._L.cns_commit_check(self._h, C.byref(ce) if ce is not None else None, C.byref(cj), C.byref(co), C.byref(ms)))
        self._commit_ms = ms.value
        return code[:j], counts

    def commit_shape(self):
        """(job_chunk, lane_max_nodes) of the check kernel: where its paths change."""
        a, b = C.c_uint32(0), C.c_uint32(0)
        self._check(self._L.cns_commit_shape(C.byref(a), C.byref(b)))
        return a.value, b.value

    def commit_timing(self) -> dict:
        """HIP-event time of the kernels of the last commit_check of this object."""
        return {"kernel_ms": getattr(self, "_commit_ms", 0.0)}

    # -- the pending gate in front of a cycle (include/crane_gpu_gate/pending_gate.h) ------------------------------------------
    def gate_pending(self, now: int, jobs: "abi.GateJobs", events: "abi.GateEvents | None" = None):
        """The dependency-event drain and Phase 1 of ScheduleThread_ (JobScheduler.cpp:1353-1413) for every job of the pending map at
        once.  -> (code, pending, ready_sec, dep_erased, counts, ev_stats): abi.GATE_* per job (the first failing check in the reference's
        order), the rows that reach NodeSelect in ascending order, the ready times after the events, 1 per dependency entry an event
        erased, the jobs per code [16], the events applied / without their pending job / without their dependency [3].  Needs a handle
        only: no snapshot, no cycle."""
        j, d = jobs.num_jobs, jobs.num_entries
        code, pending = np.zeros(max(j, 1), np.uint8), np.zeros(max(j, 1), np.uint32)
        ready, erased = np.zeros(max(j, 1), np.int64), np.zeros(max(d, 1), np.uint8)
        npend, counts, stats = np.zeros(1, np.uint64), np.zeros(16, np.uint64), np.zeros(3, np.uint64)
        cj = jobs.to_c()
        ce = events.to_c() if events is not None else None
        co = abi.CnsGateOut(abi._ptr(code), abi._ptr(pending), abi._ptr(npend), abi._ptr(ready), abi._ptr(erased), abi._ptr(counts), abi._ptr(stats))
        ms = C.c_double(0)
        self._check(self._L.cns_gate_pending(self._h, C.c_int64(now), C.byref(cj), C.byref(ce) if ce is not None else None, C.byref(co), C.byref(ms)))
        self._gate_ms = ms.value
        return code[:j], pending[:int(npend[0])], ready[:j], erased[:d], counts, stats

    def gate_shape(self):
        """(job_chunk, lane_max_deps, scan_span) of the gate's kernels: where their paths change."""
        a, b, c = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        self._check(self._L.cns_gate_shape(C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def gate_timing(self) -> dict:
        """HIP-event time of the kernels of the last gate_pending of this object."""
        return {"kernel_ms": getattr(self, "_gate_ms", 0.0)}

    # -- the submit limits over a batch of submissions (include/crane_gpu_submit/submit_limits.h) -----------------------------
    def set_submit_limits(self, tables):
        """Submit-side limits, the usage the DenyOnLimit checks read, the submit counts and the exists bits before the batch
        (submit.SubmitTables).  Needs no node snapshot."""
        t = tables.to_c()
        self._check(self._L.cns_set_submit_limits(self._h, C.byref(t)))
        self._sub_tables = tables

    def check_submissions(self, jobs: "abi.Jobs", keys, carry: bool = False):
        """TryMallocMetaSubmitResource + MallocMetaSubmitResource (AccountMetaContainer.cpp:75-153) for every job of the batch in the order
        given; job i sees the counters as jobs 0..i-1 left them.  -> (code, time_limit_out, num_admitted): abi.SUBMIT_* per job (the first
        failing check in the reference's order), the time limit after the QoS's rewrite, the number of jobs admitted.  carry: start from
        what the previous call left instead of the tables as set."""
        j = jobs.num_jobs
        if keys.num_jobs != j:
            raise ValueError("keys and jobs differ in length")
        code, tlo, adm = np.zeros(max(j, 1), np.uint8), np.zeros(max(j, 1), np.int64), np.zeros(1, np.uint64)
        cj, ck = jobs.to_c(), keys.to_c()
        co = abi.CnsSubmitOut(abi._ptr(code), abi._ptr(tlo), abi._ptr(adm))
        self._check(self._L.cns_check_submissions(self._h, C.byref(cj), C.byref(ck), C.c_uint32(abi.SUBMIT_CARRY if carry else 0), C.byref(co)))
        return code[:j], tlo[:j], int(adm[0])

    def submit_usage(self):
        """submit.SubmitState after the last check_submissions: the five submit-count tables and the three exists arrays."""
        s = self._sub_tables.state()
        self._check(self._L.cns_get_submit_usage(self._h, *s.pointers()))
        return s

    def submit_timing(self) -> dict:
        t = abi.CnsSubmitTiming()
        self._check(self._L.cns_get_submit_timing(self._h, C.byref(t)))
        return {f: getattr(t, f) for f, _ in abi.CnsSubmitTiming._fields_}

    def submit_shape(self):
        """(job_chunk, item_chunk, max_rounds): where the submit kernels' paths change."""
        a, b, c = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        self._check(self._L.cns_submit_shape(C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    # -- releases and charges on the usage tables (include/crane_gpu_usage/usage.h) ----------------------------------------------
    def set_usage_tables(self, tables):
        """The full MetaResource tables (usage.UsageTables): usage, submit counts, nested exists bytes, entity bits.  Needs no node snapshot."""
        t = tables.to_c()
        self._check(self._L.cns_usage_set_tables(self._h, C.byref(t)))
        self._use_tables = tables

    def _usage_apply(self, op, jobs, carry):
        j = jobs.num_jobs
        nf, of, clean = np.zeros(max(j, 1), np.uint16), np.zeros(max(j, 1), np.uint16), np.zeros(1, np.uint64)
        cj = jobs.to_c()
        co = abi.CnsUsageOut(abi._ptr(nf), abi._ptr(of), abi._ptr(clean))
        self._check(self._L.cns_usage_apply(self._h, C.c_uint32(op), C.byref(cj), C.c_uint32(abi.USAGE_CARRY if carry else 0), C.byref(co)))
        return nf[:j], of[:j], int(clean[0])

    def release_usage(self, jobs, carry: bool = False):
        """DoFreeResource_ (AccountMetaContainer.cpp:1126-1208) for every row of usage.UsageJobs in the order given.
        -> (not_found, over_free, num_clean): per row the records whose key was gone (:1143, :1172) / that were freed beyond what they
        held (:1152, :1196), bit layout abi.USAGE_BIT_*.  carry: start from what the previous release / charge left."""
        return self._usage_apply(abi.USAGE_RELEASE, jobs, carry)

    def charge_usage(self, jobs, carry: bool = False):
        """DoMallocResource_ (:1067-1124) for every row.  -> (not_found, over_free, num_clean): both masks zero."""
        return self._usage_apply(abi.USAGE_CHARGE, jobs, carry)

    def usage_tables(self):
        """usage.UsageState after the last release / charge (after set_usage_tables: as set, records that do not exist zeroed)."""
        s = self._use_tables.state()
        o = abi.CnsUsageTablesOut(*s.pointers())
        self._check(self._L.cns_usage_get_tables(self._h, C.byref(o)))
        return s

    def usage_timing(self) -> dict:
        t = abi.CnsUsageTiming()
        self._check(self._L.cns_usage_get_timing(self._h, C.byref(t)))
        return {f: getattr(t, f) for f, _ in abi.CnsUsageTiming._fields_}

    def usage_shape(self):
        """(job_chunk, item_chunk, carry_lanes): where the usage kernels' paths change."""
        a, b, c = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        self._check(self._L.cns_usage_shape(C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    # -- the running set kept on the device between two cycles (include/crane_gpu_running/running.h) -----------------------------
    def seed_running(self, running: "abi.Running | None", job_ids=None, attrs: "abi.RunningAttrs | None" = None):
        """The running set into the device ledger, job_ids[R] naming its rows; the per-slot running tables are derived from it on the
        device and end up exactly as set_running(running) would leave them.  After set_nodes / set_reservations.
        attrs (abi.RunningAttrs, one value per row): the ledger also carries the attribute columns (running_attrs.h); without it
        this is the plain call, which leaves a ledger without columns."""
        empty = running is None or len(running.end_sec) == 0
        if attrs is None:
            if empty:
                self._check(self._L.cns_running_seed(self._h, None, None))
                return
            ids = abi._arr(job_ids, np.uint32, len(running.end_sec))
            r = running.to_c()
            self._check(self._L.cns_running_seed(self._h, C.byref(r), abi._ptr(ids)))
            return
        if empty:
            self._check(self._L.cns_running_seed_attrs(self._h, None, None, None))
            return
        if len(attrs) != len(running.end_sec):
            raise ValueError("attrs: one value per running job")
        ids = abi._arr(job_ids, np.uint32, len(running.end_sec))
        r, a = running.to_c(), attrs.to_c()
        self._check(self._L.cns_running_seed_attrs(self._h, C.byref(r), abi._ptr(ids), C.byref(a)))

    def advance_running(self, retire_ids=(), now: "int | None" = None, job_ids=None, admit=None, reservation=None,
                        attrs: "abi.RunningAttrs | bool | None" = None):
        """One cycle boundary on the device ledger: the rows that carry one of retire_ids are erased (stably), then — when job_ids is
        given, one id per job of the last node_select's queue — every job with admit[j] != 0 (None: every job) that the cycle started at
        `now` is appended with its placements, then the per-slot running tables are rebuilt against the current layout.
        -> (found[K] uint8, num_retired, num_admitted).  Nothing to retire and nothing to admit: the rebuild alone (what follows
        set_nodes / set_reservations).
        attrs: the columns follow the rows (cns_running_advance_attrs) — an abi.RunningAttrs with one value per job of the queue when
        job_ids is given (an admitted row starts at `now`), True when there is nothing to admit.  Without it this is the plain call,
        which drops the columns."""
        ret = abi._arr(np.asarray(retire_ids, np.uint32).reshape(-1), np.uint32)
        k = len(ret)
        found, nret, nadm = np.zeros(max(k, 1), np.uint8), np.zeros(1, np.uint64), np.zeros(1, np.uint64)
        s = abi.CnsRunningStep()
        s.num_retire, s.retire_ids = k, abi._ptr(ret) if k else None
        keep = [ret]
        if job_ids is not None:
            ids = abi._arr(job_ids, np.uint32)
            s.num_jobs, s.now_sec, s.job_id = len(ids), int(now), abi._ptr(ids)
            keep.append(ids)
            if admit is not None:
                adm = abi._arr(admit, np.uint8, len(ids))
                s.admit = abi._ptr(adm)
                keep.append(adm)
            if reservation is not None:
                rv = abi._arr(reservation, np.uint32, len(ids))
                s.reservation = abi._ptr(rv)
                keep.append(rv)
        o = abi.CnsRunningStepOut(abi._ptr(found), abi._ptr(nret), abi._ptr(nadm))
        if attrs is None or attrs is False:
            self._check(self._L.cns_running_advance(self._h, C.byref(s), C.byref(o)))
        else:
            qa = attrs.to_c() if isinstance(attrs, abi.RunningAttrs) else None
            self._check(self._L.cns_running_advance_attrs(self._h, C.byref(s), C.byref(qa) if qa is not None else None, C.byref(o)))
        return found[:k], int(nret[0]), int(nadm[0])

    # -- a running job's end time changed (include/crane_gpu_amend/running_amend.h) ---------------------------------------------
    def amend_running(self, job_ids, end_sec):
        """Every ledger row whose id is job_ids[i] gets end_sec[i] (ChangeJobTimeConstraint, ResumeSuspendedJobs); the per-slot running
        tables follow when they are the ledger's.  -> (found per id, rows written)."""
        ids = abi._arr(np.asarray(job_ids, np.uint32).reshape(-1), np.uint32)
        k = len(ids)
        ends = abi._arr(np.asarray(end_sec, np.int64).reshape(-1), np.int64, k)
        found, n = np.zeros(max(k, 1), np.uint8), np.zeros(1, np.uint64)
        s = abi.CnsRunningAmend(k, abi._ptr(ids) if k else None, abi._ptr(ends) if k else None)
        o = abi.CnsRunningAmendOut(abi._ptr(found), abi._ptr(n))
        self._check(self._L.cns_running_amend_ends(self._h, C.byref(s), C.byref(o)))
        return found[:k], int(n[0])

    def running_amend_timing(self) -> dict:
        t = abi.CnsRunningAmendTiming()
        self._check(self._L.cns_running_amend_get_timing(self._h, C.byref(t)))
        return {f: getattr(t, f) for f, _ in abi.CnsRunningAmendTiming._fields_}

    def running_attrs(self) -> dict:
        """The attribute columns of the device ledger and the three values derived per row (node_num, alloc_cpu_raw, alloc_mem: what
        the sorter reads of a running job), in ledger order."""
        nj = np.zeros(1, np.uint64)
        o = abi.CnsRunningAttrsOut()
        o.num_jobs = abi._ptr(nj)
        self._check(self._L.cns_running_get_attrs(self._h, C.byref(o)))
        r = int(nj[0])
        dt = {"start_sec": np.int64, "alloc_cpu_raw": np.int64, "alloc_mem": np.uint64}
        a = {f: np.zeros(max(r, 1), dt.get(f, np.uint32)) for f, _ in abi.CnsRunningAttrsOut._fields_[2:]}
        o.capacity_jobs = r
        for f, v in a.items():
            setattr(o, f, abi._ptr(v))
        self._check(self._L.cns_running_get_attrs(self._h, C.byref(o)))
        return {f: v[:r] for f, v in a.items()}

    def priority_order_resident(self, now: int, cfg, num_accounts: int, pending, limit: "int | None" = None):
        """priority_order with the running side taken from the device ledger and its attribute columns: running job i is ledger row i.
        -> (order, priority, num_ordered), bit for bit what priority_order gives for the same rows handed in from the host."""
        J = pending.num_jobs
        order = np.empty(max(J, 1), np.uint32)
        prio = np.empty(max(J, 1), np.float64)
        nord = C.c_uint64(0)
        c_cfg, c_pd = cfg.to_c(), pending.to_c()
        self._check(self._L.cns_priority_order_resident(
            self._h, C.c_int64(now), C.byref(c_cfg), C.c_uint32(num_accounts), C.byref(c_pd), C.c_uint64(J if limit is None else limit),
            order.ctypes.data_as(C.c_void_p), prio.ctypes.data_as(C.c_void_p), C.byref(nord)))
        return order[:J], prio[:J], int(nord.value)

    def running_ledger(self):
        """The device ledger -> (abi.Running, job_ids): its rows in ledger order, every plane."""
        nj, na = np.zeros(1, np.uint64), np.zeros(1, np.uint64)
        o = abi.CnsRunningLedger()
        o.num_jobs, o.num_allocs = abi._ptr(nj), abi._ptr(na)
        self._check(self._L.cns_running_get(self._h, C.byref(o)))
        r, a = int(nj[0]), int(na[0])
        ids, end, resv, off = np.zeros(max(r, 1), np.uint32), np.zeros(max(r, 1), np.int64), np.zeros(max(r, 1), np.uint32), np.zeros(r + 1, np.uint32)
        node, cpu = np.zeros(max(a, 1), np.uint32), np.zeros(max(a, 1), np.int64)
        u64 = {f: np.zeros(max(a, 1), np.uint64) for f in ("alloc_mem", "alloc_core_lo", "alloc_core_hi", "alloc_core_w2", "alloc_core_w3", "alloc_gres")}
        o.capacity_jobs, o.capacity_allocs = r, a
        o.job_id, o.end_sec, o.reservation, o.alloc_offsets = abi._ptr(ids), abi._ptr(end), abi._ptr(resv), abi._ptr(off)
        o.alloc_node, o.alloc_cpu_raw = abi._ptr(node), abi._ptr(cpu)
        for f, v in u64.items():
            setattr(o, f, abi._ptr(v))
        self._check(self._L.cns_running_get(self._h, C.byref(o)))
        run = abi.Running(end_sec=end[:r], alloc_offsets=off, alloc_node=node[:a], alloc_cpu_raw=cpu[:a], alloc_mem=u64["alloc_mem"][:a],
                          alloc_core_lo=u64["alloc_core_lo"][:a], alloc_core_hi=u64["alloc_core_hi"][:a], alloc_gres=u64["alloc_gres"][:a],
                          reservation=resv[:r], alloc_core_w2=u64["alloc_core_w2"][:a], alloc_core_w3=u64["alloc_core_w3"][:a])
        return run, ids[:r]

    def running_timing(self) -> dict:
        t = abi.CnsRunningTiming()
        self._check(self._L.cns_running_get_timing(self._h, C.byref(t)))
        return {f: getattr(t, f) for f, _ in abi.CnsRunningTiming._fields_}

    def running_shape(self):
        """(job_chunk, lane_max_allocs, sort_tile, scan_span): where the running ledger's kernels change path."""
        v = [C.c_uint32(0) for _ in range(4)]
        self._check(self._L.cns_running_shape(*[C.byref(x) for x in v]))
        return tuple(x.value for x in v)

    # -- a cycle with preemption on that set (include/crane_gpu_running/running_preempt.h) ---------------------------------------
    def node_select_preempt_resident(self, now: int, jobs: abi.Jobs, preempt: "abi.Preempt", from_attrs: bool = False):
        """node_select_preempt for a handle whose running tables were built by seed_running / advance_running; -> (Placements,
        PreemptOut).  LEDGER ORDER: running job index r is ledger row r, so preempt.rn_job_id / rn_qos / rn_qos_priority / rn_start_sec
        are in the ledger's order (seed order, stable erase, admitted jobs appended in queue order; running_ledger() reports it), and a
        reference without bit 31 in the preempted lists is a ledger row.  rn_job_id is checked against the ledger on the device.
        advance_running behind it needs its admit mask.
        from_attrs: cns_running_select_preempt_attrs — the running jobs' qos, qos_priority and start_sec come from the ledger's columns
        and preempt's rn_* arrays are not handed in at all (leave them empty)."""
        out = abi.Placements(jobs.num_jobs, jobs.total_places())
        cj, co, cp = jobs.to_c(), out.to_c(), preempt.to_c()
        if from_attrs:
            nj = np.zeros(1, np.uint64)
            led = abi.CnsRunningLedger()
            led.num_jobs = abi._ptr(nj)
            self._check(self._L.cns_running_get(self._h, C.byref(led)))
            pout = abi.PreemptOut(jobs.num_jobs, int(nj[0]))
            cpo = pout.to_c()
            if preempt.enabled:
                cp.rn_job_id = cp.rn_qos = cp.rn_qos_priority = cp.rn_start_sec = None
            self._check(self._L.cns_running_select_preempt_attrs(self._h, C.c_int64(now), C.byref(cj), C.byref(cp), C.byref(co), C.byref(cpo)))
            self._jobs = jobs
            return out, pout
        pout = abi.PreemptOut(jobs.num_jobs, len(preempt.rn_job_id))
        cpo = pout.to_c()
        self._check(self._L.cns_running_select_preempt(self._h, C.c_int64(now), C.byref(cj), C.byref(cp), C.byref(co), C.byref(cpo)))
        self._jobs = jobs
        return out, pout

    def preempt_index(self) -> dict:
        """The index the last node_select_preempt_resident ran on, as built on the device: ent_job, ent_slot, ent_end (the patched per-slot
        end times) per entry; rj_off [rows + 1], rj_ent per entry, rj_end and rj_preempting per ledger row."""
        ne, nr = np.zeros(1, np.uint64), np.zeros(1, np.uint64)
        o = abi.CnsPreemptIndexOut()
        o.num_entries, o.num_rows = abi._ptr(ne), abi._ptr(nr)
        self._check(self._L.cns_debug_get_preempt_index(self._h, C.byref(o)))
        m, r = int(ne[0]), int(nr[0])
        a = {"ent_job": np.zeros(max(m, 1), np.uint32), "ent_slot": np.zeros(max(m, 1), np.uint32), "ent_end": np.zeros(max(m, 1), np.int64),
             "rj_off": np.zeros(r + 1, np.uint32), "rj_ent": np.zeros(max(m, 1), np.uint32), "rj_end": np.zeros(max(r, 1), np.int64),
             "rj_preempting": np.zeros(max(r, 1), np.uint8)}
        o.capacity_entries, o.capacity_rows = m, r
        for f, v in a.items():
            setattr(o, f, abi._ptr(v))
        self._check(self._L.cns_debug_get_preempt_index(self._h, C.byref(o)))
        return {f: v[:(r + 1 if f == "rj_off" else r if f in ("rj_end", "rj_preempting") else m)] for f, v in a.items()}

    def preempt_setup_timing(self) -> dict:
        """What the last cycle with preemption (either call) spent in front of its cycle: setup_ms on the host clock, index_ms / mark_ms on
        the device (node_select_preempt_resident only)."""
        t = abi.CnsRunningPreemptTiming()
        self._check(self._L.cns_running_preempt_get_timing(self._h, C.byref(t)))
        return {f: getattr(t, f) for f, _ in abi.CnsRunningPreemptTiming._fields_}

    def device_results(self):
        p, n = C.c_void_p(), C.c_uint64()
        self._check(self._L.cns_device_results(self._h, C.byref(p), C.byref(n)))
        return p.value, n.value

    # -- one process per device: the all-gather of the packed results over RCCL (csrc/group_host.inc) ----------------
    def results_layout(self) -> dict:
        """Byte offsets of the packed result buffer of the last upload (cns_results_layout)."""
        o = abi.CnsResultsOffsets()
        self._check(self._L.cns_results_layout(self._h, C.byref(o)))
        return {f: getattr(o, f) for f, _ in abi.CnsResultsOffsets._fields_}

    @staticmethod
    def comm_unique_id() -> bytes:
        """rank 0: the communicator's id (ship it to every rank: torch.distributed's store, MPI, a file)"""
        buf = (C.c_uint8 * 128)()
        rc = lib().cns_comm_unique_id(buf)
        if rc != 0:
            raise EngineError(rc, (lib().cns_last_error(None) or b"").decode())
        return bytes(buf)

    def comm_init_rank(self, nranks: int, rank: int, uid: bytes):
        buf = (C.c_uint8 * 128).from_buffer_copy(uid)
        self._check(self._L.cns_comm_init_rank(self._h, C.c_uint32(nranks), C.c_uint32(rank), buf))

    def comm_destroy(self):
        self._check(self._L.cns_comm_destroy(self._h))

    def allgather_results(self, slot_bytes: int) -> int:
        """collective: every rank's packed results, rank r at [r * slot_bytes) of a device buffer of this engine -> its address"""
        p = C.c_void_p()
        self._check(self._L.cns_allgather_results(self._h, C.c_uint64(slot_bytes), C.byref(p)))
        return p.value

    def download_gathered(self, nbytes: int) -> np.ndarray:
        out = np.empty(nbytes, np.uint8)
        self._check(self._L.cns_download_gathered(self._h, out.ctypes.data_as(C.c_void_p), C.c_uint64(nbytes)))
        return out

    def gather_timing(self):
        ms, b = C.c_double(), C.c_uint64()
        self._L.cns_gather_timing(self._h, C.byref(ms), C.byref(b))
        return ms.value, b.value

    def timing(self) -> dict:
        t = abi.CnsTiming()
        self._check(self._L.cns_get_timing(self._h, C.byref(t)))
        return {f: getattr(t, f) for f, _ in abi.CnsTiming._fields_}

    def last_kernel(self) -> str:
        """Selection kernel of the last run: 'k_pipe<NPL>' (decoupled test / commit pipeline) or 'k_select<NPL>'."""
        return (self._L.cns_debug_last_kernel(self._h) or b"").decode()

    # -- parity helpers ------------------------------------------------------------------------------
    def costs(self) -> np.ndarray:
        c = np.zeros(len(self._cluster.part_nodes), np.float64)
        self._check(self._L.cns_debug_get_costs(self._h, c.ctypes.data_as(C.c_void_p)))
        return c

    def prof(self) -> np.ndarray:
        """[P, 32] cycle counters of the last run (zeros unless built with -DCNS_PROF)."""
        P = self._cluster.num_partitions
        out = np.zeros(P * 32, np.uint64)
        self._check(self._L.cns_debug_get_prof(self._h, out.ctypes.data_as(C.c_void_p), C.c_uint32(P * 32)))
        return out.reshape(P, 32)

    WIDE_STATS = ("looks_empty", "looks_consumed", "leader_polls_ring_full", "stops", "flushes", "redo_with_exclusion",
                  "serial_jobs", "resource_verdicts", "partitions_straddling_xcds",
                  "windows", "jobs_decided_in_windows", "windows_that_decided_nothing", "prefetch_wave_gave_up",   # (round 5: several jobs per exchange, wide_kernel.inc)
                  "home_workgroups")   # (round 6: summed over the partitions — 8 partitions x 3 homes = 24)

    def wide_stats(self) -> dict:
        """Always-on protocol counters of k_wide's last run, summed over the partitions (every build; zeros for the other
        kernels): who waited for whom (supervisor looks without / with a decision, leader polls in front of a full ring) and
        how often the chain was broken (stops, flushes) and mended (redo with an excluded candidate, serial jobs, "Resource")."""
        self._L.cns_debug_engine_partitions.restype = C.c_uint32
        P = int(self._L.cns_debug_engine_partitions(self._h)) or self._cluster.num_partitions   # (groups of partitions that share nodes + reservations)
        out = np.zeros(P * 48, np.uint64)
        self._check(self._L.cns_debug_get_prof(self._h, out.ctypes.data_as(C.c_void_p), C.c_uint32(P * 48)))
        st = out[P * 32:].reshape(P, 16).sum(axis=0)
        return {k: int(v) for k, v in zip(self.WIDE_STATS, st)}

    def timeline(self, node: int, cap: int = 1100):
        n = C.c_uint32(0)
        t = np.zeros(cap, np.int64); cpu = np.zeros(cap, np.int64)
        mem = np.zeros(cap, np.uint64); lo = np.zeros(cap, np.uint64)
        hi = np.zeros(cap, np.uint64); g = np.zeros(cap, np.uint64)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        self._check(self._L.cns_debug_get_timeline(self._h, C.c_uint32(node), C.c_uint32(cap), C.byref(n),
                                                   p(t), p(cpu), p(mem), p(lo), p(hi), p(g)))
        k = min(n.value, cap)
        w2 = np.zeros(cap, np.uint64); w3 = np.zeros(cap, np.uint64)
        self._check(self._L.cns_debug_get_timeline_cores(self._h, C.c_uint32(node), C.c_uint32(cap), p(w2), p(w3)))
        return {"t": t[:k], "cpu_raw": cpu[:k], "mem": mem[:k], "core_lo": lo[:k], "core_hi": hi[:k], "gres": g[:k],
                "core_w2": w2[:k], "core_w3": w3[:k]}


class GpuNodeSelectorGroup:
    """ONE process, N devices (cns_group_*: what the C++ adapter's GpuNodeSelectionAlgo(std::vector<int> devices) drives): the groups of
    partitions dealt over the devices, every shard on its own host thread, the packed results all-gathered on the devices (RCCL when the
    devices are distinct) and merged back into queue order.  A repeated ordinal ([0, 0]) exercises the path on a one-GPU box."""

    def __init__(self, devices, scheduled_batch_size: int = 0, max_job_num_per_node: int = 0, max_time_window_sec: int = 0):
        self._L = lib()
        self._g = C.c_void_p()
        cfg = abi.CnsConfig(abi.CNS_ABI_VERSION, 0, scheduled_batch_size, max_job_num_per_node, 0, max_time_window_sec)
        dev = (C.c_int32 * len(devices))(*devices)
        rc = self._L.cns_group_create(C.byref(cfg), dev, C.c_uint32(len(devices)), C.byref(self._g))
        if rc != 0:
            msg = self._L.cns_group_last_error(None)
            self._g = C.c_void_p()
            raise EngineError(rc, msg.decode() if msg else "")
        self._cluster = None

    def _check(self, rc: int):
        if rc != 0:
            msg = self._L.cns_group_last_error(self._g)
            raise EngineError(rc, msg.decode() if msg else "")

    def close(self):
        if self._g:
            self._L.cns_group_destroy(self._g)
            self._g = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_nodes(self, cluster: abi.Cluster):
        c = cluster.to_c()
        self._check(self._L.cns_group_set_nodes(self._g, C.byref(c)))
        self._cluster = cluster

    def set_reservations(self, reservations):
        if reservations is None:
            self._check(self._L.cns_group_set_reservations(self._g, None))
        else:
            r = reservations.to_c()
            self._check(self._L.cns_group_set_reservations(self._g, C.byref(r)))

    def set_running(self, running):
        if running is None:
            self._check(self._L.cns_group_set_running(self._g, None))
        else:
            r = running.to_c()
            self._check(self._L.cns_group_set_running(self._g, C.byref(r)))

    def node_select(self, now: int, jobs: abi.Jobs, out: "abi.Placements | None" = None) -> abi.Placements:
        if out is None:
            out = abi.Placements(jobs.num_jobs, jobs.total_places())
        cj, co = jobs.to_c(), out.to_c()
        self._check(self._L.cns_group_select(self._g, C.c_int64(now), C.byref(cj), C.byref(co)))
        return out

    def info(self) -> dict:
        i = abi.CnsGroupInfo()
        self._check(self._L.cns_group_get_info(self._g, C.byref(i)))
        d = {f: getattr(i, f) for f, _ in abi.CnsGroupInfo._fields_}
        d["gather_mode"] = {1: "rccl", 2: "device-copies"}.get(d["gather_mode"], d["gather_mode"])
        return d

    def device_of_partition(self, p: int) -> int:
        return int(self._L.cns_group_device_of_partition(self._g, C.c_uint32(p)))

    def partition_status(self) -> np.ndarray:
        """cns_partition_status per partition of the caller (0: served), whichever device it was dealt to."""
        st = np.zeros(self._cluster.num_partitions, np.uint8)
        self._check(self._L.cns_group_get_partition_status(self._g, st.ctypes.data_as(C.c_void_p), C.c_uint32(len(st))))
        return st

    def last_kernels(self):
        n = self._L.cns_group_size(self._g)
        return [(self._L.cns_debug_last_kernel(self._L.cns_group_handle(self._g, d)) or b"").decode() for d in range(n)]

    def costs_of_device(self, d: int, n: int) -> np.ndarray:
        c = np.zeros(n, np.float64)
        h = self._L.cns_group_handle(self._g, d)
        rc = self._L.cns_debug_get_costs(C.c_void_p(h), c.ctypes.data_as(C.c_void_p))
        if rc != 0:
            raise EngineError(rc, (self._L.cns_last_error(C.c_void_p(h)) or b"").decode())
        return c
