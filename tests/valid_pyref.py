"""The truth of include/crane_gpu_valid/validity.h: a Python restatement of the partition checks of JobScheduler::CheckJobValidity
(src/CraneCtld/JobScheduler.cpp:7262-7374) with the resource algebra it calls (src/Utilities/PublicHeader/PublicHeader.cpp:619-659 and
:57-69), the reference's line beside every statement.  Plain Python integers and dicts, one job and one node at a time, nothing shared with
the engine's packed words.  CheckJobValidity hangs on the Ctld singletons, so it is restated, not sliced; tests/test_valid_pyref.py holds this
file to hand-derived cases.

Model: a GRES map is {name: GresCount}, GresCount = (total, {type: count}); a type is the class index of the layout, a name its name id.
A zero count is no entry (validity.h, input rules).  A node's dedicated GRES is {name: {type: slots}} with the types it HAS slots of."""
from __future__ import annotations

import numpy as np

from cranesched_amd import abi

I64_MAX, U64_MAX = 2 ** 63 - 1, 2 ** 64 - 1
RESV_NONE = 0xFFFFFFFF


def node_gres(cluster: abi.Cluster, n: int) -> dict:
    """name -> {type: slot count} of res_total[n] (DedicatedResourceInNode::name_type_slots_map)."""
    g, out = cluster.gres, {}
    m = int(cluster.gres_slots[n])
    for c in range(len(g.class_name)):
        cnt = bin(m & g.class_mask(c)).count("1")
        if cnt:
            out.setdefault(int(g.class_name[c]), {})[c] = cnt
    return out


def job_gres(cluster: abi.Cluster, jobs: abi.Jobs, j: int) -> dict:
    """name -> (total, {type: specified}) of req_node_res_view; a class the layout does not define is a type of a name nobody has."""
    g, out = cluster.gres, {}
    if jobs.gres_total is not None:
        for k in range(abi.MAX_GRES_NAMES):
            if int(jobs.gres_total[j, k]):
                out[k] = [int(jobs.gres_total[j, k]), {}]
    if jobs.gres_spec is not None:
        for c in range(abi.MAX_GRES_CLASSES):
            s = int(jobs.gres_spec[j, c])
            if s:
                name = int(g.class_name[c]) if c < len(g.class_name) else ("undefined", c)
                out.setdefault(name, [0, {}])[1][c] = s
    return out


def gres_count_le(lhs, rhs) -> bool:
    """operator<=(GresCount, GresCount), PublicHeader.cpp:57-69."""
    if lhs[0] > rhs[0]:                         # :59
        return False
    for t, cnt in lhs[1].items():               # :62
        if t not in rhs[1]:                     # :63-64
            return False
        if cnt > rhs[1][t]:                     # :65
            return False
    return True                                 # :68


def view_le_view(lhs, rhs) -> bool:
    """operator<=(ResourceView, ResourceView), PublicHeader.cpp:648-659.  A view = (cpu, mem, gres map)."""
    if lhs[0] > rhs[0]:                         # :649
        return False
    if lhs[1] > rhs[1]:                         # :650
        return False
    for name, gc in lhs[2].items():             # :652
        if name not in rhs[2]:                  # :653-654
            return False
        if not gres_count_le(gc, rhs[2][name]):  # :655
            return False
    return True                                 # :658


def view_le_node(lhs, cpu, mem, gres) -> bool:
    """operator<=(ResourceView, ResourceInNodeV3), PublicHeader.cpp:619-646."""
    if lhs[0] > cpu:                            # :620
        return False
    if lhs[1] > mem:                            # :621
        return False
    for name, gc in lhs[2].items():             # :625
        if name not in gres:                    # :626-627
            return False
        types = gres[name]                      # :629
        for t, cnt in gc[1].items():            # :632
            if t not in types:                  # :633-634
                return False
            if cnt > types[t]:                  # :635
                return False
        if gc[0] > sum(types.values()):         # :639-642
            return False
    return True                                 # :645


def partition_total(cluster: abi.Cluster, p: int):
    """res_total_inc_dead of partition p: the sum of res_total over every listed node (CranedMetaContainer.cpp:364-391), as a view.
    (cpu and mem saturate at INT64_MAX / UINT64_MAX: validity.h.)"""
    cpu = mem = 0
    gres = {}
    for n in cluster.part_nodes[int(cluster.part_offsets[p]):int(cluster.part_offsets[p + 1])]:
        cpu += int(cluster.cpu_total_raw[n])
        mem += int(cluster.mem_total[n])
        for name, types in node_gres(cluster, int(n)).items():
            gc = gres.setdefault(name, [0, {}])
            for t, cnt in types.items():
                gc[0] += cnt
                gc[1][t] = gc[1].get(t, 0) + cnt
    return (min(cpu, I64_MAX), min(mem, U64_MAX), gres)


def check(cluster: abi.Cluster, jobs: abi.Jobs, resv_nodes=None):
    """-> (code [J] uint8, eligible [J] uint32).  resv_nodes: per reservation the set of its nodes (None: no reservation)."""
    J, P, N = jobs.num_jobs, cluster.num_partitions, cluster.num_nodes
    V = 0 if resv_nodes is None else len(resv_nodes)
    code, elig = np.zeros(J, np.uint8), np.zeros(J, np.uint32)
    totals, refused, ngres = {}, {}, {}
    for j in range(J):
        k, nt = int(jobs.node_num[j]), int(jobs.ntasks[j])
        ncpu = int(jobs.node_cpu_raw[j]) if jobs.node_cpu_raw is not None else 0
        tcpu, nmem, tmem = int(jobs.task_cpu_raw[j]), int(jobs.node_mem[j]), int(jobs.task_mem[j])
        g = job_gres(cluster, jobs, j)
        tot_cpu, tot_mem = ncpu * k + tcpu * nt, nmem * k + tmem * nt             # :7156-7157
        one_cpu, one_mem = ncpu + tcpu, nmem + tmem                               # :7356
        if (k == 0 or nt < k or tot_mem > U64_MAX or one_mem > U64_MAX or
                not -I64_MAX - 1 <= tot_cpu <= I64_MAX or not -I64_MAX - 1 <= one_cpu <= I64_MAX or
                not -I64_MAX - 1 <= ncpu * k <= I64_MAX or not -I64_MAX - 1 <= tcpu * nt <= I64_MAX):
            code[j] = abi.VALID_BAD_REQUEST
            continue
        if tot_mem == 0:                                                          # :7262
            code[j] = abi.VALID_ZERO_MEM
            continue
        if tcpu == 0:                                                             # :7266
            code[j] = abi.VALID_ZERO_CPU
            continue
        p = int(jobs.partition[j])
        if p >= P:                                                                # :7278
            code[j] = abi.VALID_PARTITION_NOT_FOUND
            continue
        nodes = [int(n) for n in cluster.part_nodes[int(cluster.part_offsets[p]):int(cluster.part_offsets[p + 1])]]
        if p not in totals:
            totals[p] = partition_total(cluster, p)
            refused[p] = cluster.unsupported is not None and any(cluster.unsupported[n] for n in nodes)
        if refused[p]:
            code[j] = abi.VALID_REFUSED
            continue
        req_total = (tot_cpu, tot_mem, {name: [gc[0] * k, {t: c * k for t, c in gc[1].items()}] for name, gc in g.items()})   # :7156, GresCount::operator*= :45-51
        if not view_le_view(req_total, totals[p]):                                # :7283
            code[j] = abi.VALID_NO_RESOURCE
            continue
        if k > len(nodes):                                                        # :7299
            code[j] = abi.VALID_NODE_NUM
            continue
        incl = excl = None
        if jobs.incl_offsets is not None:
            incl = [int(x) for x in jobs.incl_nodes[int(jobs.incl_offsets[j]):int(jobs.incl_offsets[j + 1])]]
        if jobs.excl_offsets is not None:
            excl = [int(x) for x in jobs.excl_nodes[int(jobs.excl_offsets[j]):int(jobs.excl_offsets[j + 1])]]
        rsv = int(jobs.reservation[j]) if jobs.reservation is not None else RESV_NONE
        if rsv != RESV_NONE:                                                      # :7307
            if rsv >= V:                                                          # :7308
                code[j] = abi.VALID_RESV_NOT_FOUND
                continue
            if incl and any(n not in resv_nodes[rsv] for n in incl):              # :7338-7349
                code[j] = abi.VALID_RESV_NODE
                continue
        req_one = (one_cpu, one_mem, g)
        avail = 0
        for n in nodes:                                                           # :7354
            if n not in ngres:
                ngres[n] = node_gres(cluster, n)
            if (view_le_node(req_one, int(cluster.cpu_total_raw[n]), int(cluster.mem_total[n]), ngres[n])   # :7356-7357
                    and (not incl or n in incl)                                   # :7358-7359
                    and (not excl or n not in excl)):                             # :7360-7361
                avail += 1                                                        # :7362 (the full count: :7364's break is not taken)
        elig[j] = avail
        code[j] = abi.VALID_NOT_ENOUGH_NODES if k > avail else abi.VALID_OK       # :7368, :7376
    return code, elig


def resv_node_sets(resv: "abi.Reservations | None"):
    if resv is None:
        return None
    return [set(int(n) for n in resv.alloc_node[int(resv.alloc_offsets[v]):int(resv.alloc_offsets[v + 1])]) for v in range(resv.num_resv)]
