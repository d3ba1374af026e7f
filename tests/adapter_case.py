"""String-level cases for the C++ adapter (cranesched_amd/host): GpuNodeSelectionAlgo against the oracle, job by job.

`to_case` turns an ABI scenario (helpers.random_case, test_reservations.random_resv_case, test_overlap.overlap_case, synth.make_config /
make_loaded) into the objects CraneCtld hands the adapter — CranedMeta, partitions, ResvMeta, RnJobInScheduler, PdJobInScheduler — with
string names that set the traps a string layer falls into (node names whose string order is not their dense order, a GRES class of 12
slots whose ids sort differently as strings and as numbers, two types under one name, memory_sw_bytes != memory_bytes, drained and dead
nodes, a node in no partition, unknown nodes in include / exclude lists, unknown partitions, reservations, GRES names and types, preset
reasons).

`derive` builds, from those objects alone and from the reference's rules (not from the adapter), the ABI arrays the oracle consumes:
  * dense node index = position in craned_metas; schedulable = alive && !drain (JobScheduler.cpp:6595);
  * GRES classes in (name, type) order, a class as wide as the union of its slot ids over all nodes, bits in string order of the slot
    ids: std::set<SlotId>, whose lowest ids are taken first (PublicHeader.cpp:565-578);
  * the untyped remainder of a request over several types is taken in class order.  The reference leaves that order to an
    unordered_map (PublicHeader.cpp:582-592); class order is the project's canonical order.
`expected` turns oracle placements into the objects NodeSelect must leave behind (JobScheduler.cpp:6300-6331, 6745-6831).
"""
from __future__ import annotations

import json
import os
import subprocess

import numpy as np

from cranesched_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "cranesched_amd", "host", "test_host_adapter")
GIB = 1 << 30
UNKNOWN_NODE = 0xFFFFFFFE      # an include list's name that is no node (cns_job_soa::incl_nodes)
UNKNOWN_RESV = 0xFFFFFFFE      # a reservation name that is no reservation -> "Reservation Not Found"
REASON_TEXT = {abi.REASON_NONE: "", abi.REASON_PRIORITY: "Priority", abi.REASON_RESOURCE: "Resource",
               abi.REASON_RESOURCE_RESERVED: "Resource Reserved", abi.REASON_PARTITION_NOT_FOUND: "Partition Not Found",
               abi.REASON_RESERVATION_NOT_FOUND: "Reservation Not Found", 7: "Preempted",
               abi.REASON_ENGINE_REFUSED: "GpuEngineRefused"}
GRES_NAMES = ["gpu", "npu", "fpga", "nic"]
QOS_NAMES = ["normal", "high", "critical", "low"]   # qos id -> name: string order is not id order
GRES_TYPES = [["a100", "h100", "l40", "mi300"], ["a910", "b910"], ["u55"], ["cx7"]]


def _ids(*words):
    out = []
    for w, word in enumerate(words):
        word = int(word)
        while word:
            b = word & -word
            out.append(64 * w + b.bit_length() - 1)
            word ^= b
    return out


def _bits(mask: int):
    out = []
    while mask:
        b = mask & -mask
        out.append(b.bit_length() - 1)
        mask ^= b
    return out


class Case:
    """The objects of one NodeSelect call, as plain Python values."""

    def __init__(self, now):
        self.now = int(now)
        self.nodes = []        # dict(name, alive, drain, res)
        self.partitions = []   # (name, [node names])
        self.resvs = []        # dict(name, start, end, res={node: res})
        self.running = []      # dict(id, qos, qos_priority, resv, start, end, res={node: res})
        self.pending = []      # dict(id, partition, resv, L, k, nt, tmin, tmax, excl, reason, qos, qos_priority, node_req, task_req, incl, excl_nodes)
        self.preempt = (False, {})

    # ---- file form (read by test_host_adapter's read_case) ------------------------------------------------------------------------------
    @staticmethod
    def _s(x):
        return x if x else "-"

    def _res(self, r):
        t = [r["cpu"], r["mem"], r["msw"], len(r["cores"]), *r["cores"]]
        items = [(n, ty, sl) for n, tm in sorted(r["gres"].items()) for ty, sl in sorted(tm.items())]
        t.append(len(items))
        for n, ty, sl in items:
            t += [n, ty, len(sl), *sorted(sl)]
        return t

    def _req(self, q):
        t = [q["cpu"], q["mem"], q["msw"], len(q["gres"])]
        for name, (total, spec) in q["gres"].items():
            t += [name, total, len(spec)]
            for ty, c in spec.items():
                t += [ty, c]
        return t

    def text(self) -> str:
        L = [f"now {self.now}", f"nodes {len(self.nodes)}"]
        for n in self.nodes:
            L.append(" ".join(map(str, [n["name"], int(n["alive"]), int(n["drain"]), *self._res(n["res"])])))
        L.append(f"partitions {len(self.partitions)}")
        for name, names in self.partitions:
            L.append(" ".join(map(str, [name, len(names), *names])))
        L.append(f"resvs {len(self.resvs)}")
        for v in self.resvs:
            t = [v["name"], v["start"], v["end"], len(v["res"])]
            for cid, r in v["res"].items():
                t += [cid, *self._res(r)]
            L.append(" ".join(map(str, t)))
        L.append(f"running {len(self.running)}")
        for r in self.running:
            t = [r["id"], self._s(r["qos"]), r["qos_priority"], self._s(r["resv"]), r["start"], r["end"], len(r["res"])]
            for cid, x in r["res"].items():
                t += [cid, *self._res(x)]
            L.append(" ".join(map(str, t)))
        L.append(f"pending {len(self.pending)}")
        for p in self.pending:
            t = [p["id"], self._s(p["partition"]), self._s(p["resv"]), p["L"], p["k"], p["nt"], p["tmin"], p["tmax"], int(p["excl"]),
                 self._s(p["reason"]), self._s(p["qos"]), p["qos_priority"], float(p.get("priority", 0.0)).hex(), *self._req(p["node_req"]), *self._req(p["task_req"]),
                 len(p["incl"]), *p["incl"], len(p["excl_nodes"]), *p["excl_nodes"]]
            L.append(" ".join(map(str, t)))
        en, table = self.preempt
        L.append(f"preempt {int(en)} {len(table)}")
        for q, lst in table.items():
            L.append(" ".join(map(str, [q, len(lst), *lst])))
        return "\n".join(L) + "\n"

    def write(self, path):
        with open(path, "w") as f:
            f.write(self.text())


# ---------------------------------------------------------------------------------------------------------------------------------------
# ABI scenario -> string case, with the traps
# ---------------------------------------------------------------------------------------------------------------------------------------
def to_case(cluster: abi.Cluster, jobs: abi.Jobs, now: int, running: abi.Running | None = None,
            resv: abi.Reservations | None = None, seed: int = 0, traps: bool = True, pre: abi.Preempt | None = None,
            plain: bool = False) -> Case:
    """pre: QoS preemption (test_preempt.random_preempt_case) as QoS names, a preempt table and the jobs' QoS fields.
    plain: slot ids whose string order is their bit order and no trap, so that the derived arrays ARE the scenario's arrays."""
    traps = traps and not plain
    rng = np.random.default_rng(7000 + seed)
    N = cluster.num_nodes
    lay = cluster.gres
    # node i is "cn<perm[i] + 1>": the dense order is neither the string order nor the numeric order of the names
    perm = rng.permutation(N)
    names = [f"cn{int(perm[i]) + 1}" for i in range(N)]
    # GRES class c -> (name, type); the first class of a name with 12 slot ids over the nodes (/dev/nvidia0..11: /dev/nvidia10 sorts
    # before /dev/nvidia2), the others with ids of their own
    per_name = {}
    cls_key = []
    for c in range(len(lay.class_name)):
        nm = int(lay.class_name[c])
        t = per_name.get(nm, 0)
        per_name[nm] = t + 1
        cls_key.append((GRES_NAMES[nm], GRES_TYPES[nm][t]))

    def slot(c, b, n):
        w = int(lay.class_width[c])
        if plain:
            return f"/dev/{cls_key[c][1]}_{b:02d}"
        if c == 0:
            return f"/dev/nvidia{b + w * (n % 3)}"
        return f"/dev/{cls_key[c][1]}_{b}"

    def res_of(cpu, mem, msw, words, g, n):
        gres = {}
        for c in range(len(lay.class_name)):
            bits = (int(g) >> int(lay.class_shift[c])) & ((1 << int(lay.class_width[c])) - 1)
            if bits:
                gres.setdefault(cls_key[c][0], {})[cls_key[c][1]] = [slot(c, b, n) for b in _bits(bits)]
        return {"cpu": int(cpu), "mem": int(mem), "msw": int(msw), "cores": _ids(*words), "gres": gres}

    def w(arr, i):
        return 0 if arr is None else int(arr[i])

    case = Case(now)
    sched = cluster.schedulable if cluster.schedulable is not None else np.ones(N, np.uint8)
    n_off = 0
    for i in range(N):
        alive, drain = True, False
        if not sched[i]:   # not schedulable: dead and drained in turn
            alive, drain = (False, False) if n_off % 2 == 0 else (True, True)
            n_off += 1
        elif traps and i % 17 == 5:
            drain = True
        elif traps and i % 17 == 11:
            alive = False
        mem = int(cluster.mem_total[i])
        case.nodes.append({"name": names[i], "alive": alive, "drain": drain,
                           "res": res_of(cluster.cpu_total_raw[i], mem, mem // 2 + (i + 1) * 4096,
                                         [cluster.core_lo[i], cluster.core_hi[i], w(cluster.core_w2, i), w(cluster.core_w3, i)],
                                         cluster.gres_slots[i], i)})
    orphan = None
    if traps:   # a node in no partition, dense last, string first
        orphan = "cn0"
        case.nodes.append({"name": orphan, "alive": True, "drain": False,
                           "res": {"cpu": 64 * 256, "mem": 256 * GIB, "msw": 3 * GIB, "cores": list(range(64)), "gres": {}}})
    P = cluster.num_partitions
    pnames = [f"part{p}" for p in range(P)]
    for p in range(P):
        a, b = int(cluster.part_offsets[p]), int(cluster.part_offsets[p + 1])
        case.partitions.append((pnames[p], [names[int(x)] for x in cluster.part_nodes[a:b]]))
    V = resv.num_resv if resv is not None else 0
    vnames = [f"resv{v}" for v in range(V)]
    for v in range(V):
        a, b = int(resv.alloc_offsets[v]), int(resv.alloc_offsets[v + 1])
        rr = {}
        for q in range(a, b):
            n = int(resv.alloc_node[q])
            rr[names[n]] = res_of(resv.alloc_cpu_raw[q], resv.alloc_mem[q], int(resv.alloc_mem[q]) // 3,
                                  [resv.alloc_core_lo[q], resv.alloc_core_hi[q], w(resv.alloc_core_w2, q), w(resv.alloc_core_w3, q)],
                                  resv.alloc_gres[q], n)
        case.resvs.append({"name": vnames[v], "start": int(resv.start_sec[v]), "end": int(resv.end_sec[v]), "res": rr})
    if running is not None:
        for r in range(len(running.end_sec)):
            a, b = int(running.alloc_offsets[r]), int(running.alloc_offsets[r + 1])
            rr = {}
            for q in range(a, b):
                n = int(running.alloc_node[q])
                rr[names[n]] = res_of(running.alloc_cpu_raw[q], running.alloc_mem[q], int(running.alloc_mem[q]) + 5,
                                      [running.alloc_core_lo[q], running.alloc_core_hi[q], w(running.alloc_core_w2, q),
                                       w(running.alloc_core_w3, q)], running.alloc_gres[q], n)
            rv = int(running.reservation[r]) if running.reservation is not None else abi.RESV_NONE
            case.running.append({"id": 1_000_000 + r, "qos": QOS_NAMES[int(pre.rn_qos[r])] if pre is not None else "normal",
                                 "qos_priority": int(pre.rn_qos_priority[r]) if pre is not None else 0, "resv": vnames[rv] if rv < V else "",
                                 "start": int(pre.rn_start_sec[r]) if pre is not None else now - 100, "end": int(running.end_sec[r]), "res": rr})
        if traps and case.running:   # a running job with a record on a node the snapshot does not know, one in an unknown reservation
            case.running[0]["res"]["ghost1"] = {"cpu": 256, "mem": GIB, "msw": GIB, "cores": [0], "gres": {}}
            case.running.append({"id": 1_000_000 + len(case.running), "qos": "", "qos_priority": 0, "resv": "noresv",
                                 "start": now - 10, "end": now + 500, "res": {names[0]: {"cpu": 256, "mem": GIB, "msw": 0, "cores": [0], "gres": {}}}})
    J = jobs.num_jobs
    part_of = {}
    for p, (pn, lst) in enumerate(case.partitions):
        for x in lst:
            part_of.setdefault(x, set()).add(pn)
    presets = ["License", "Held", "Dependency"]
    for j in range(J):
        p = int(jobs.partition[j])
        rv = int(jobs.reservation[j]) if jobs.reservation is not None else abi.RESV_NONE
        node_gres = {}
        if jobs.gres_total is not None:
            for nm in range(abi.MAX_GRES_NAMES):
                tot = int(jobs.gres_total[j, nm])
                spec = {}
                for c in range(len(lay.class_name)):
                    if int(lay.class_name[c]) == nm and int(jobs.gres_spec[j, c]):
                        spec[cls_key[c][1]] = int(jobs.gres_spec[j, c])
                if tot or spec:
                    node_gres[GRES_NAMES[nm]] = (tot, spec)
        excl = bool(jobs.exclusive[j]) if jobs.exclusive is not None else False
        incl, exn = [], []
        if jobs.incl_offsets is not None:
            incl = [names[int(x)] for x in jobs.incl_nodes[int(jobs.incl_offsets[j]):int(jobs.incl_offsets[j + 1])]]
            exn = [names[int(x)] for x in jobs.excl_nodes[int(jobs.excl_offsets[j]):int(jobs.excl_offsets[j + 1])]]
        reason = ""
        if jobs.skip is not None and jobs.skip[j]:
            reason = presets[j % len(presets)]
        node_cpu = int(jobs.node_cpu_raw[j]) if jobs.node_cpu_raw is not None else 0
        nmem = int(jobs.node_mem[j])
        tmem = int(jobs.task_mem[j])
        case.pending.append({"id": j + 1, "partition": pnames[p] if p < P else "nopart", "resv": (vnames[rv] if rv < V else "noresv") if rv != abi.RESV_NONE else "",
                             "L": int(jobs.time_limit_sec[j]), "k": int(jobs.node_num[j]), "nt": int(jobs.ntasks[j]),
                             "tmin": int(jobs.ntasks_per_node_min[j]), "tmax": int(jobs.ntasks_per_node_max[j]), "excl": excl,
                             "reason": reason, "qos": QOS_NAMES[int(pre.pd_qos[j])] if pre is not None else "normal",
                             "qos_priority": int(pre.pd_qos_priority[j]) if pre is not None else 0,
                             "priority": float(pre.pd_priority[j]) if pre is not None else 0.0,
                             "node_req": {"cpu": node_cpu, "mem": nmem, "msw": nmem // 2 + 17, "gres": node_gres},
                             "task_req": {"cpu": int(jobs.task_cpu_raw[j]), "mem": tmem, "msw": tmem + 3 * 1024, "gres": {}},
                             "incl": incl, "excl_nodes": exn})
    if pre is not None:   # qos id q -> QOS_NAMES[q]; a QoS the table does not know ("guest") preempts nothing and is preempted by nobody
        case.preempt = (True, {QOS_NAMES[q]: [QOS_NAMES[x] for x in lst] for q, lst in enumerate(pre.qos_preempt)})
        for x, p in enumerate(case.pending):
            if x % 23 == 7:
                p["qos"] = "guest"
        for x, r in enumerate(case.running):
            if x % 11 == 3:
                r["qos"] = "guest"
    if traps and J:
        r = np.random.default_rng(8000 + seed)
        pick = r.choice(J, size=min(J, 40), replace=False)
        for x, j in enumerate(pick):
            p = case.pending[int(j)]
            if p["reason"]:
                continue
            kind = x % 8
            if kind == 0:      # include list: an unknown node and the orphan (outside every partition) next to real ones
                p["incl"] = p["incl"] + ["ghost2", orphan]
            elif kind == 1:    # include list of unknown nodes only: can never be met
                p["incl"] = ["ghost3"]
            elif kind == 2:    # exclude list naming unknown nodes (and a real one)
                p["excl_nodes"] = p["excl_nodes"] + ["ghost4", names[int(r.integers(0, N))]]
            elif kind == 3:    # a GRES name no node carries
                p["node_req"]["gres"]["tpu"] = (1, {})
            elif kind == 4:    # a GRES type no node carries, under a name that exists
                p["node_req"]["gres"]["gpu"] = (1, {"v100": 1})
            elif kind == 5:    # an unknown partition name
                p["partition"] = "nopart"
            elif kind == 6:    # an unknown reservation name
                p["resv"] = "noresv"
            elif kind == 7:    # include list naming a node of the partition and a node of another one
                if incl_ok := [n["name"] for n in case.nodes[:N] if pnames and p["partition"] in part_of.get(n["name"], ())]:
                    p["incl"] = [incl_ok[0], orphan]
    return case


# ---------------------------------------------------------------------------------------------------------------------------------------
# string case -> ABI arrays, from the reference's rules (not from the adapter)
# ---------------------------------------------------------------------------------------------------------------------------------------
class Derived:
    pass


def _masks(cores):
    w = [0, 0, 0, 0]
    for c in cores:
        assert c < 256, "core ids >= 256 are outside these cases"
        w[c // 64] |= 1 << (c % 64)
    return w


def derive(case: Case, running_order: str = "case", preempting=()) -> Derived:
    """running_order "id": the running jobs in ascending job id (the event-fed mirror: the reference's running-job map order).
    preempting: m_preempting_set_ as the previous cycle on the same object left it."""
    d = Derived()
    N = len(case.nodes)
    d.node_names = [n["name"] for n in case.nodes]
    idx = {n: i for i, n in enumerate(d.node_names)}
    d.node_index = idx
    # GRES classes: (name, type) order; width = union of slot ids over all nodes; bits in std::set<std::string> order
    union = {}
    for n in case.nodes:
        for name, tm in n["res"]["gres"].items():
            for ty, sl in tm.items():
                union.setdefault((name, ty), set()).update(sl)
    d.classes = sorted(union)
    assert len(d.classes) <= abi.MAX_GRES_CLASSES
    name_ids = {}
    shift = 0
    d.slot_bit, d.bit_slot = {}, {}
    cn, cs, cw = [], [], []
    for (name, ty) in d.classes:
        name_ids.setdefault(name, len(name_ids))
        slots = sorted(union[(name, ty)])
        cn.append(name_ids[name]); cs.append(shift); cw.append(len(slots))
        for b, s in enumerate(slots):
            d.slot_bit[(name, ty, s)] = shift + b
            d.bit_slot[shift + b] = (name, ty, s)
        shift += len(slots)
    assert shift <= 64 and len(name_ids) <= abi.MAX_GRES_NAMES
    d.name_ids = name_ids
    d.layout = abi.GresLayout(class_name=cn, class_shift=cs, class_width=cw)
    d.class_of = {k: c for c, k in enumerate(d.classes)}

    def gmask(gres):
        m = 0
        for name, tm in gres.items():
            for ty, sl in tm.items():
                for s in sl:
                    b = d.slot_bit.get((name, ty, s))
                    if b is not None:
                        m |= 1 << b
        return m

    def rec(r):
        w = _masks(r["cores"])
        return [r["cpu"], r["mem"], *w, gmask(r["gres"])]

    nodes = [rec(n["res"]) for n in case.nodes]
    arr = lambda col, dt: np.array([x[col] for x in nodes], dt) if nodes else np.zeros(0, dt)
    d.msw = [n["res"]["msw"] for n in case.nodes]
    sched = np.array([1 if (n["alive"] and not n["drain"]) else 0 for n in case.nodes], np.uint8)
    poff, pnodes = [0], []
    d.part_index = {}
    for name, lst in case.partitions:
        d.part_index[name] = len(poff) - 1
        pnodes += [idx[x] for x in lst if x in idx]
        poff.append(len(pnodes))
    d.cluster = abi.Cluster(arr(0, np.int64), arr(1, np.uint64), arr(2, np.uint64), arr(3, np.uint64), arr(6, np.uint64),
                            np.array(poff, np.uint32), np.array(pnodes, np.uint32), gres=d.layout, schedulable=sched,
                            core_w2=arr(4, np.uint64), core_w3=arr(5, np.uint64), unsupported=np.zeros(N, np.uint8))
    # reservations
    d.resv_index = {v["name"]: i for i, v in enumerate(case.resvs)}
    d.resv = None
    d.resv_recs = []
    if case.resvs:
        off, recs = [0], []
        for v in case.resvs:
            recs += [[idx[c], *rec(r)] for c, r in v["res"].items() if c in idx]
            off.append(len(recs))
            d.resv_recs.append(sorted(tuple(x) for x in recs[off[-2]:off[-1]]))
        col = lambda k, dt: np.array([x[k] for x in recs], dt)
        d.resv = abi.Reservations([v["start"] for v in case.resvs], [v["end"] for v in case.resvs], off, col(0, np.uint32), col(1, np.int64),
                                  col(2, np.uint64), col(3, np.uint64), col(4, np.uint64), col(7, np.uint64),
                                  alloc_core_w2=col(5, np.uint64), alloc_core_w3=col(6, np.uint64))
    # running jobs: a job in an unknown reservation is in no node state (JobScheduler.cpp:6692-6707); records on unknown nodes drop
    rjobs = list(case.running)
    if running_order == "id":
        rjobs.sort(key=lambda r: r["id"])
    end, rres, off, recs = [], [], [0], []
    d.run_recs, d.run_ids, run_objs = [], [], []
    for r in rjobs:
        if r["resv"] and r["resv"] not in d.resv_index:
            continue
        end.append(r["end"]); rres.append(d.resv_index[r["resv"]] if r["resv"] else abi.RESV_NONE)
        recs += [[idx[c], *rec(x)] for c, x in r["res"].items() if c in idx]
        off.append(len(recs))
        d.run_recs.append(sorted(tuple(x) for x in recs[off[-2]:off[-1]]))
        d.run_ids.append(r["id"])
        run_objs.append(r)
    d.running = None
    if end:
        col = lambda k, dt: np.array([x[k] for x in recs], dt)
        d.running = abi.Running(end, off, col(0, np.uint32), col(1, np.int64), col(2, np.uint64), col(3, np.uint64), col(4, np.uint64),
                                col(7, np.uint64), reservation=rres, alloc_core_w2=col(5, np.uint64), alloc_core_w3=col(6, np.uint64))
    d.run_end, d.run_resv = end, rres
    # pending jobs
    J = len(case.pending)
    gtot = np.zeros((J, abi.MAX_GRES_NAMES), np.uint8)
    gspec = np.zeros((J, abi.MAX_GRES_CLASSES), np.uint8)
    part, jres, incl_off, incl, exo, exn = [], [], [0], [], [0], []
    d.incl_lists, d.excl_lists = [], []
    for j, p in enumerate(case.pending):
        part.append(d.part_index.get(p["partition"], 0xFFFFFFFF))        # -> "Partition Not Found"
        jres.append(d.resv_index.get(p["resv"], UNKNOWN_RESV) if p["resv"] else abi.RESV_NONE)
        absent = False
        for name, (tot, spec) in p["node_req"]["gres"].items():
            if name not in name_ids:          # a name no node carries: never fits (ABI: 255 of name 0, whatever else is asked)
                absent = absent or bool(tot or spec)
                continue
            gtot[j, name_ids[name]] = min(tot, 255)
            for ty, c in spec.items():
                if (name, ty) not in d.class_of:   # a type no node carries
                    if c:
                        gtot[j, name_ids[name]] = 255
                    continue
                gspec[j, d.class_of[(name, ty)]] = min(c, 127)
        if absent:
            gtot[j, 0] = 255
        # included_nodes / excluded_nodes are sets of names: one entry per distinct name, in no particular order
        il = [idx.get(x, UNKNOWN_NODE) for x in dict.fromkeys(p["incl"])]
        incl += il; incl_off.append(len(incl))
        d.incl_lists.append(sorted(il))
        el = [idx[x] for x in dict.fromkeys(p["excl_nodes"]) if x in idx]
        exn += el; exo.append(len(exn))
        d.excl_lists.append(sorted(el))
    col = lambda key, dt: np.array([p[key] for p in case.pending], dt)
    sub = lambda req, key, dt: np.array([p[req][key] for p in case.pending], dt)
    d.jobs = abi.Jobs(partition=np.array(part, np.uint32), time_limit_sec=col("L", np.int64), node_mem=sub("node_req", "mem", np.uint64),
                      task_cpu_raw=sub("task_req", "cpu", np.int64), task_mem=sub("task_req", "mem", np.uint64), node_num=col("k", np.uint32),
                      ntasks=col("nt", np.uint32), ntasks_per_node_min=col("tmin", np.uint32), ntasks_per_node_max=col("tmax", np.uint32),
                      node_cpu_raw=sub("node_req", "cpu", np.int64), exclusive=col("excl", np.uint8), gres_total=gtot, gres_spec=gspec,
                      incl_offsets=np.array(incl_off, np.uint64), incl_nodes=np.array(incl or [0], np.uint32),
                      excl_offsets=np.array(exo, np.uint64), excl_nodes=np.array(exn or [0], np.uint32),
                      skip=np.array([1 if p["reason"] else 0 for p in case.pending], np.uint8), reservation=np.array(jres, np.uint32))
    # preemption (JobScheduler.cpp:6532-6543: the preempt lists of the QoS table; a QoS it does not know preempts nothing)
    d.preempt = None
    en, table = case.preempt
    if en:
        qid = {}
        for q in sorted(table):
            qid.setdefault(q, len(qid))
        for q in [p["qos"] for p in case.pending] + [r["qos"] for r in run_objs]:
            qid.setdefault(q, len(qid))
        lists = [[] for _ in qid]
        for q, lst in table.items():
            lists[qid[q]] = [qid.setdefault(x, len(qid)) for x in lst]
        lists += [[] for _ in range(len(qid) - len(lists))]
        d.preempt = abi.Preempt(lists, [p["id"] for p in case.pending], [qid[p["qos"]] for p in case.pending],
                                [p["qos_priority"] for p in case.pending], [p.get("priority", 0.0) for p in case.pending],
                                [r["id"] for r in run_objs], [qid[r["qos"]] for r in run_objs], [r["qos_priority"] for r in run_objs],
                                [r["start"] for r in run_objs], preempting=sorted(preempting))
    d.pending_ids = [p["id"] for p in case.pending]
    return d


def oracle_select(d: Derived, now: int, batch: int = 0, backend: str = "oracle", with_preempt: bool = False):
    """-> Placements, or (Placements, PreemptOut | None) with with_preempt"""
    from oracle import pyoracle
    run = pyoracle.select(d.cluster, d.jobs, now, running=d.running, reservations=d.resv, scheduled_batch_size=batch,
                          preempt=d.preempt, backend=backend)
    return (run.placements, getattr(run, "preempt_out", None)) if with_preempt else run.placements


# ---------------------------------------------------------------------------------------------------------------------------------------
# oracle placements -> the objects NodeSelect leaves behind
# ---------------------------------------------------------------------------------------------------------------------------------------
def expected(case: Case, d: Derived, pl: abi.Placements, mode: str = "lazy", po=None):
    """mode lazy (default write-back): a job backfilled for later carries reason, start_time and end_time only; full
    (SetFullWriteBack(true)): also its placement, as the reference leaves it (JobScheduler.cpp:6345-6368); deferred: as lazy once
    MaterializeAllocation has run for every job that starts now.  po (PreemptOut): preempted_jobs as (kind, job id) in push order, the
    pending queue index / running-table index of the oracle mapped back to job ids."""
    out = []
    lists = po.lists() if po is not None else None
    for j, p in enumerate(case.pending):
        e = {"job": p["id"], "reason": p["reason"], "start": 0, "end": 0, "craned_ids": [], "task_num": {}, "alloc": {}, "preempted": []}
        out.append(e)
        if lists is not None:
            e["preempted"] = [["P", d.pending_ids[i]] if is_pd else ["R", d.run_ids[i]] for is_pd, i in lists[j]]
        r = int(pl.reason[j])
        if r == abi.REASON_SKIPPED:        # the caller's reason stays (cpp:6744)
            continue
        e["reason"] = REASON_TEXT[r]
        st = int(pl.start_sec[j])
        if st == 0:                        # "Leave start_time unset" (cpp:6769-6771)
            continue
        e["start"], e["end"] = st, st + p["L"]   # cpp:6772
        if mode != "full" and r != abi.REASON_NONE:
            continue
        a, b = int(pl.place_offsets[j]), int(pl.place_offsets[j + 1])
        for q in range(a, b):
            n = int(pl.node_idx[q])
            if n == abi.NODE_NONE:
                continue
            cid = d.node_names[n]
            e["craned_ids"].append(cid)
            e["task_num"][cid] = int(pl.ntasks[q])
            gres = {}
            for bit in _bits(int(pl.gres[q])):
                name, ty, s = d.bit_slot[bit]
                gres.setdefault(name, {}).setdefault(ty, []).append(s)
            for tm in gres.values():
                for ty in tm:
                    tm[ty] = sorted(tm[ty])
            # an exclusive job gets the node's whole res_total, memory_sw_bytes included (cpp:6309-6310)
            msw = d.msw[n] if p["excl"] else p["node_req"]["msw"] + p["task_req"]["msw"] * int(pl.ntasks[q])
            e["alloc"][cid] = {"cpu": int(pl.cpu_raw[q]), "mem": int(pl.mem[q]), "msw": msw,
                               "cores": _ids(pl.core_lo[q], pl.core_hi[q], pl.core_w2[q], pl.core_w3[q]), "gres": gres}
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# the driver
# ---------------------------------------------------------------------------------------------------------------------------------------
def run_driver(args, timeout=300):
    r = subprocess.run([EXE, *map(str, args)], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), f"{args}: rc {r.returncode}\n{r.stdout}\n{r.stderr}"
    return r


def read_pack(path):
    out = {}
    with open(path) as f:
        for line in f:
            t = line.split()
            if t:
                out[t[0]] = [int(x) for x in t[1:]]
    return out


def read_dump(path):
    with open(path) as f:
        rows = [json.loads(x) for x in f if x.strip()]
    tail = rows[-1] if rows and "status" in rows[-1] else None
    return [x for x in rows if "job" in x], tail


def write_placements(pl: abi.Placements, path):
    J = pl.num_jobs
    L = [str(J)]
    for j in range(J):
        a, b = int(pl.place_offsets[j]), int(pl.place_offsets[j + 1])
        L.append(f"{int(pl.start_sec[j])} {int(pl.reason[j])} {b - a}")
        for q in range(a, b):
            L.append(" ".join(str(int(x)) for x in (pl.node_idx[q], pl.ntasks[q], pl.cpu_raw[q], pl.mem[q], pl.core_lo[q], pl.core_hi[q],
                                                    pl.gres[q], pl.core_w2[q], pl.core_w3[q])))
    with open(path, "w") as f:
        f.write("\n".join(L) + "\n")


def u64(a):
    return [int(x) & 0xFFFFFFFFFFFFFFFF for x in np.asarray(a).reshape(-1).tolist()]


def compare_pack(got: dict, d: Derived):
    """The adapter's packed arrays == the derived ones, array for array.  Per-job record lists of running jobs and reservations and
    include lists come from unordered containers: compared as sorted lists."""
    c = d.cluster
    exp = {"n_cpu": c.cpu_total_raw, "n_mem": c.mem_total, "n_lo": c.core_lo, "n_hi": c.core_hi, "n_w2": c.core_w2, "n_w3": c.core_w3,
           "n_gres": c.gres_slots, "n_sched": c.schedulable, "n_unsup": c.unsupported, "part_offsets": c.part_offsets,
           "part_nodes": c.part_nodes, "layout_num_classes": [len(d.layout.class_name)], "layout_class_name": d.layout.class_name,
           "layout_class_shift": d.layout.class_shift, "layout_class_width": d.layout.class_width}
    jb = d.jobs
    exp.update({"j_part": jb.partition, "j_L": jb.time_limit_sec, "j_ncpu": jb.node_cpu_raw, "j_nmem": jb.node_mem, "j_tcpu": jb.task_cpu_raw,
                "j_tmem": jb.task_mem, "j_k": jb.node_num, "j_nt": jb.ntasks, "j_tmin": jb.ntasks_per_node_min,
                "j_tmax": jb.ntasks_per_node_max, "j_excl": jb.exclusive, "j_skip": jb.skip, "j_resv": jb.reservation,
                "j_gtot": jb.gres_total, "j_gspec": jb.gres_spec, "j_ioff": jb.incl_offsets, "j_eoff": jb.excl_offsets,
                "r_end": d.run_end, "r_resv": d.run_resv})
    exp["v_start"] = d.resv.start_sec if d.resv is not None else []
    exp["v_end"] = d.resv.end_sec if d.resv is not None else []
    for k, v in exp.items():
        assert k in got, f"the adapter does not report {k}"
        assert got[k] == u64(v), f"{k} differs: adapter {got[k][:16]}... vs derived {u64(v)[:16]}..."
    # include / exclude lists, per job, as sets (they come from unordered sets)
    for key, lists in (("i", d.incl_lists), ("e", d.excl_lists)):
        off = got[f"j_{key}off"]
        for j, want in enumerate(lists):
            assert sorted(got[f"j_{key}nodes"][off[j]:off[j + 1]]) == u64(want), f"{key} list of job {j} differs"

    def per_job(prefix, offk, recs_exp):
        off = got[offk]
        keys = ("node", "cpu", "mem", "lo", "hi", "w2", "w3", "g")
        cols = [got[f"{prefix}_{k}"] for k in keys]
        assert len(off) == len(recs_exp) + 1, f"{prefix}: {len(off) - 1} jobs vs {len(recs_exp)}"
        for j, want in enumerate(recs_exp):
            have = sorted(tuple(col[q] for col in cols) for q in range(off[j], off[j + 1]))
            assert have == [tuple(u64(x)) for x in want], f"{prefix} records of entry {j} differ:\n{have}\n{want}"

    per_job("r", "r_off", d.run_recs)
    per_job("v", "v_off", d.resv_recs)

