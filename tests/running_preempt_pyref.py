"""The index of a cycle with preemption over the running ledger (include/crane_gpu_running/running_preempt.h) in plain Python and numpy:
the per-slot entry order as cns_set_running derives it from the ledger (snapshot_host.inc: build_running), then ent_job / ent_slot,
the job -> entries CSR, the preempting marks, the patched ends, rj_end and set_in, written as the host loops of cns_select_preempt read
(preempt_host.inc: running_side).  Inputs: a ledger (tests/running_pyref.py), the layout's node -> slots map, the reservations' slot
ranges, `now` and the preempting set.  layout_of() states the slot layout of a snapshot whose partitions are all served (snapshot_host.inc: build_layout,
build_resv).  This is the truth cns_debug_get_preempt_index is held to — never the code under test."""
from __future__ import annotations

import numpy as np

from cranesched_amd import abi


def layout_of(cluster: abi.Cluster, reservations: "abi.Reservations | None" = None):
    """-> (node_slots: per node the list of its slots, resv_slots: per reservation (first slot, its nodes ascending)).
    Partitions connected through shared nodes form one group; groups stand in the order of their first partition, inside a group the
    member partitions in ascending order, each with its schedulable nodes ascending: one slot per (member partition, node).  Behind
    them every reservation's virtual slots, its nodes ascending."""
    N, P = cluster.num_nodes, cluster.num_partitions
    sched = np.ones(N, bool) if cluster.schedulable is None else np.asarray(cluster.schedulable).astype(bool)
    lists = [sorted({int(n) for n in cluster.part_nodes[int(cluster.part_offsets[p]):int(cluster.part_offsets[p + 1])] if sched[int(n)]}) for p in range(P)]
    root = list(range(P))

    def find(x):
        while root[x] != x:
            x = root[x]
        return x

    first = {}
    for p in range(P):
        for n in lists[p]:
            if n in first:
                a, b = find(first[n]), find(p)
                if a != b:
                    root[max(a, b)] = min(a, b)
            else:
                first[n] = p
    groups, seen = [], {}
    for p in range(P):
        r = find(p)
        if r not in seen:
            seen[r] = len(groups)
            groups.append([])
        groups[seen[r]].append(p)
    node_slots = [[] for _ in range(N)]
    q = 0
    for g in groups:
        for p in g:
            for n in lists[p]:
                node_slots[n].append(q)
                q += 1
    resv_slots = []
    if reservations is not None:
        for v in range(len(reservations.start_sec)):
            nodes = sorted(int(n) for n in reservations.alloc_node[int(reservations.alloc_offsets[v]):int(reservations.alloc_offsets[v + 1])])
            resv_slots.append((q, nodes))
            q += len(nodes)
    return node_slots, resv_slots


def slots_of(row, node, node_slots, resv_slots):
    """The slots an allocation of `row` on `node` counts on: every slot of the node (none: not schedulable, JobScheduler.cpp:6685-6686),
    or inside a reservation its virtual slot there (none: unknown reservation, or it does not list the node, :6693-6700)."""
    if row.reservation == abi.RESV_NONE:
        return list(node_slots[node])
    if row.reservation >= len(resv_slots):
        return []
    first, nodes = resv_slots[row.reservation]
    return [first + nodes.index(node)] if node in nodes else []


def entry_order(ledger, node_slots, resv_slots):
    """build_running's entries: [(slot, ledger row)], grouped by slot ascending, inside a slot in ledger order."""
    per_slot = {}
    for r, row in enumerate(ledger.rows):
        for node, _ in row.allocs:
            for q in slots_of(row, node, node_slots, resv_slots):
                per_slot.setdefault(q, []).append(r)
    return [(q, r) for q in sorted(per_slot) for r in per_slot[q]]


def index(ledger, node_slots, resv_slots, now, preempting):
    """-> dict: ent_job, ent_slot, ent_end, rj_off, rj_ent, rj_end, rj_preempting as numpy arrays, and set_in (a list)."""
    ents = entry_order(ledger, node_slots, resv_slots)
    R, A = len(ledger.rows), len(ents)
    ent_slot = np.array([q for q, _ in ents], np.uint32)
    ent_job = np.array([r for _, r in ents], np.uint32)
    rn_end = np.array([ledger.rows[r].end_sec for _, r in ents], np.int64)
    # m_preempting_set_: ids that no longer run are dropped, the others end at now + 1 (JobScheduler.cpp:6545-6559)
    id_to_rn = {}
    for r, row in enumerate(ledger.rows):
        id_to_rn.setdefault(row.job_id, r)
    rj_pre = np.zeros(R, np.uint8)
    set_in = []
    for i in preempting:
        if int(i) not in id_to_rn:
            continue
        rj_pre[id_to_rn[int(i)]] = 1
        set_in.append(int(i))
    rj_off = np.zeros(R + 1, np.uint32)
    for d in range(A):
        rj_off[ent_job[d] + 1] += 1
    for r in range(R):
        rj_off[r + 1] += rj_off[r]
    rj_ent = np.zeros(A, np.uint32)
    cur = [int(x) for x in rj_off[:-1]]
    for d in range(A):
        rj_ent[cur[ent_job[d]]] = d
        cur[ent_job[d]] += 1
    ent_end = rn_end.copy()
    rj_end = np.zeros(R, np.int64)
    for d in range(A):
        r = int(ent_job[d])
        if rj_pre[r]:
            ent_end[d] = now + 1
        rj_end[r] = max(int(ent_end[d]), now + 1)   # :6513-6514
    return dict(ent_job=ent_job, ent_slot=ent_slot, ent_end=ent_end, rj_off=rj_off, rj_ent=rj_ent, rj_end=rj_end, rj_preempting=rj_pre,
                set_in=sorted(set(set_in)))


INDEX_FIELDS = ("ent_job", "ent_slot", "ent_end", "rj_off", "rj_ent", "rj_end", "rj_preempting")


def same_index(got, want):
    """None, or the first table in which a downloaded index differs from index()."""
    for f in INDEX_FIELDS:
        a, b = np.asarray(got[f]), np.asarray(want[f])
        if a.shape != b.shape or not np.array_equal(a.astype(np.int64), b.astype(np.int64)):
            return f
    return None
