"""Cases of the validity check (include/crane_gpu_valid/validity.h): a hand-derived table and a seeded generator.
Shared by tests/test_valid_pyref.py (CPU: the truth is held to the table, the generator to its mix) and tests/test_gpu_validity.py."""
from __future__ import annotations

import functools

import numpy as np

from cranesched_amd import abi

G = 1 << 30
CORE = 256          # cpu raw units per core
NONE = 0xFFFFFFFF

# (name, type) classes: gpu/a100 bits 0..3, gpu/v100 bits 4..7, fpga/x bits 8..9
LAYOUT = abi.GresLayout(class_name=[0, 0, 1], class_shift=[0, 4, 8], class_width=[4, 4, 2])
A100, V100, FPGA_X = 0, 1, 2
GPU, FPGA = 0, 1


def make_cluster(nodes, parts, layout=LAYOUT) -> abi.Cluster:
    """nodes: (cores, mem, gres mask, schedulable, unsupported); parts: node lists."""
    cores = [n[0] for n in nodes]
    off = np.concatenate([[0], np.cumsum([len(p) for p in parts])])
    flat = [x for p in parts for x in p]
    unsup = [n[4] for n in nodes]
    return abi.Cluster(cpu_total_raw=[c * CORE for c in cores], mem_total=[n[1] for n in nodes],
                       core_lo=[(1 << min(c, 64)) - 1 if c < 64 else 2 ** 64 - 1 for c in cores], core_hi=[0] * len(nodes),
                       gres_slots=[n[2] for n in nodes], part_offsets=off, part_nodes=np.asarray(flat, np.uint32), gres=layout,
                       schedulable=[n[3] for n in nodes], unsupported=unsup if any(unsup) else None)


def make_resv(cluster: abi.Cluster, node_lists) -> abi.Reservations:
    """Reservations over the given nodes, one core and 1 GiB of each (only the node lists matter to the validity check)."""
    off = np.concatenate([[0], np.cumsum([len(v) for v in node_lists])])
    flat = [n for v in node_lists for n in v]
    m = len(flat)
    return abi.Reservations(start_sec=[1000] * len(node_lists), end_sec=[2000] * len(node_lists), alloc_offsets=off, alloc_node=flat,
                            alloc_cpu_raw=[CORE] * m, alloc_mem=[G] * m, alloc_core_lo=[1] * m, alloc_core_hi=[0] * m, alloc_gres=[0] * m)


def make_jobs(rows) -> abi.Jobs:
    """rows: dicts with p, tcpu (raw), tmem, and optionally ncpu, nmem, k, nt, tmin, gt {name: n}, gs {class: n}, incl, excl, rsv."""
    J = len(rows)
    gt, gs = np.zeros((J, 4), np.uint8), np.zeros((J, 8), np.uint8)
    ioff, eoff, incl, excl = [0], [0], [], []
    for j, r in enumerate(rows):
        for a, b in r.get("gt", {}).items():
            gt[j, a] = b
        for a, b in r.get("gs", {}).items():
            gs[j, a] = b
        incl += list(r.get("incl", ()))
        excl += list(r.get("excl", ()))
        ioff.append(len(incl))
        eoff.append(len(excl))
    k = [r.get("k", 1) for r in rows]
    tmin = [r.get("tmin", 1) for r in rows]
    return abi.Jobs(partition=[r["p"] for r in rows], time_limit_sec=[3600] * J, node_mem=[r.get("nmem", 0) for r in rows],
                    task_cpu_raw=[r["tcpu"] for r in rows], task_mem=[r["tmem"] for r in rows], node_num=k,
                    ntasks=[r.get("nt", r.get("k", 1)) for r in rows], ntasks_per_node_min=tmin, ntasks_per_node_max=[max(t, 64) for t in tmin],
                    node_cpu_raw=[r.get("ncpu", 0) for r in rows], gres_total=gt, gres_spec=gs, incl_offsets=ioff,
                    incl_nodes=np.asarray(incl, np.uint32), excl_offsets=eoff, excl_nodes=np.asarray(excl, np.uint32),
                    reservation=[r.get("rsv", NONE) for r in rows])


# ---- the hand-derived table ------------------------------------------------------------------------------------------------------------
# nodes:  n0 8c 16G | n1 8c 16G DOWN | n2 16c 64G a100 x2 | n3 16c 64G a100 x1 + v100 x2 | n4 4c 8G | n5 4c 8G UNSUPPORTED | n6 8c 16G fpga x1
# p0 = {n0 n1 n2 n3}: 48c 160G, gpu 5 (a100 3, v100 2)    p1 = {n3 n4}: 20c 72G, gpu 3 (a100 1, v100 2)
# p2 = {n4 n5}: lists the unsupported node                 p3 = {n6}: 8c 16G, fpga 1
# reservation 0 = {n2 n3}
HAND_NODES = [(8, 16 * G, 0, 1, 0), (8, 16 * G, 0, 0, 0), (16, 64 * G, 0b11, 1, 0), (16, 64 * G, 0b110001, 1, 0),
              (4, 8 * G, 0, 1, 0), (4, 8 * G, 0, 1, 1), (8, 16 * G, 1 << 8, 1, 0)]
HAND_PARTS = [[0, 1, 2, 3], [3, 4], [4, 5], [6]]
HAND_RESV = [[2, 3]]
C = abi
# (what it shows, job, code, eligible)
HAND = [
    ("node_num 0", dict(p=0, tcpu=CORE, tmem=G, k=0, nt=1), C.VALID_BAD_REQUEST, 0),
    ("ntasks < node_num", dict(p=0, tcpu=CORE, tmem=G, k=2, nt=1), C.VALID_BAD_REQUEST, 0),
    ("task_mem * ntasks overflows", dict(p=0, tcpu=CORE, tmem=1 << 63, k=1, nt=2), C.VALID_BAD_REQUEST, 0),
    ("node_cpu + task_cpu overflows", dict(p=0, ncpu=2 ** 63 - 1, tcpu=CORE, tmem=G), C.VALID_BAD_REQUEST, 0),
    ("zero memory (before zero cpu)", dict(p=0, tcpu=0, tmem=0), C.VALID_ZERO_MEM, 0),
    ("zero cpu (before the partition is looked at)", dict(p=99, tcpu=0, tmem=G), C.VALID_ZERO_CPU, 0),
    ("no such partition", dict(p=4, tcpu=CORE, tmem=G), C.VALID_PARTITION_NOT_FOUND, 0),
    ("a reservation job whose partition index is invalid", dict(p=9, tcpu=CORE, tmem=G, rsv=0), C.VALID_PARTITION_NOT_FOUND, 0),
    ("the partition lists an unsupported node", dict(p=2, tcpu=CORE, tmem=G), C.VALID_REFUSED, 0),
    ("... sharing n4 with it refuses nobody", dict(p=1, tcpu=CORE, tmem=G), C.VALID_OK, 2),
    ("ntasks_per_node_min 4 on nodes that hold one task", dict(p=0, tcpu=8 * CORE, tmem=G, k=1, nt=4, tmin=4), C.VALID_OK, 4),
    ("the down node n1 counts: 4 of 4", dict(p=0, tcpu=8 * CORE, tmem=16 * G, k=4, nt=4), C.VALID_OK, 4),
    ("cpu and mem exactly res_total (and exactly the partition's)", dict(p=3, tcpu=8 * CORE, tmem=16 * G), C.VALID_OK, 1),
    ("cpu exactly a node's", dict(p=0, tcpu=16 * CORE, tmem=G), C.VALID_OK, 2),
    ("... one raw unit more", dict(p=0, tcpu=16 * CORE + 1, tmem=G), C.VALID_NOT_ENOUGH_NODES, 0),
    ("mem exactly a node's", dict(p=0, tcpu=CORE, tmem=64 * G), C.VALID_OK, 2),
    ("... one byte more", dict(p=0, tcpu=CORE, tmem=64 * G + 1), C.VALID_NOT_ENOUGH_NODES, 0),
    ("total cpu exactly the partition's", dict(p=1, tcpu=CORE, tmem=G, k=1, nt=20), C.VALID_OK, 2),
    ("... one raw unit more", dict(p=1, ncpu=1, tcpu=CORE, tmem=G, k=1, nt=20), C.VALID_NO_RESOURCE, 0),
    ("total mem exactly the partition's", dict(p=1, tcpu=64, tmem=G, k=1, nt=72), C.VALID_OK, 2),
    ("... one byte more", dict(p=1, nmem=1, tcpu=64, tmem=G, k=1, nt=72), C.VALID_NO_RESOURCE, 0),
    ("a specified type no node of the partition has", dict(p=3, tcpu=CORE, tmem=G, gs={A100: 1}), C.VALID_NO_RESOURCE, 0),
    ("a specified type of a class the layout does not define", dict(p=0, tcpu=CORE, tmem=G, gs={5: 1}), C.VALID_NO_RESOURCE, 0),
    ("a specified count above any node's", dict(p=0, tcpu=CORE, tmem=G, gs={A100: 200}), C.VALID_NO_RESOURCE, 0),
    ("a specified type in the partition, on too few nodes", dict(p=0, tcpu=CORE, tmem=G, k=2, nt=2, gs={V100: 1}), C.VALID_NOT_ENOUGH_NODES, 1),
    ("an untyped total served across types (n3: 1 + 2)", dict(p=0, tcpu=CORE, tmem=G, gt={GPU: 3}), C.VALID_OK, 1),
    ("an untyped total no single node has", dict(p=0, tcpu=CORE, tmem=G, gt={GPU: 4}), C.VALID_NOT_ENOUGH_NODES, 0),
    ("a name the partition does not have", dict(p=0, tcpu=CORE, tmem=G, gt={FPGA: 1}), C.VALID_NO_RESOURCE, 0),
    ("total and specified together", dict(p=0, tcpu=CORE, tmem=G, gt={GPU: 2}, gs={A100: 2}), C.VALID_OK, 1),
    ("an include list names a node outside the partition", dict(p=1, tcpu=CORE, tmem=G, incl=[0, 4]), C.VALID_OK, 1),
    ("... and two nodes are asked for", dict(p=1, tcpu=CORE, tmem=G, k=2, nt=2, incl=[0, 4]), C.VALID_NOT_ENOUGH_NODES, 1),
    ("an include entry beyond the node table", dict(p=1, tcpu=CORE, tmem=G, incl=[1000, 4]), C.VALID_OK, 1),
    ("an exclude list removes the last eligible node", dict(p=3, tcpu=CORE, tmem=G, excl=[6]), C.VALID_NOT_ENOUGH_NODES, 0),
    ("an exclude entry outside the partition removes nothing", dict(p=3, tcpu=CORE, tmem=G, excl=[0, 70000]), C.VALID_OK, 1),
    ("include and exclude lists together", dict(p=0, tcpu=CORE, tmem=G, incl=[0, 2, 3], excl=[2]), C.VALID_OK, 2),
    ("an excluded node that does not fit was never counted", dict(p=0, tcpu=16 * CORE, tmem=G, excl=[0, 2]), C.VALID_OK, 1),
    ("node_num == eligible", dict(p=0, tcpu=16 * CORE, tmem=G, k=2, nt=2), C.VALID_OK, 2),
    ("node_num == eligible + 1", dict(p=0, tcpu=16 * CORE, tmem=G, k=3, nt=3), C.VALID_NOT_ENOUGH_NODES, 2),
    ("more nodes than the partition lists", dict(p=3, tcpu=CORE, tmem=G, k=2, nt=2), C.VALID_NODE_NUM, 0),
    ("... comes before the reservation is looked up", dict(p=0, tcpu=CORE, tmem=G, k=9, nt=9, rsv=5), C.VALID_NODE_NUM, 0),
    ("no such reservation", dict(p=0, tcpu=CORE, tmem=G, rsv=1), C.VALID_RESV_NOT_FOUND, 0),
    ("an included node outside the reservation", dict(p=0, tcpu=CORE, tmem=G, rsv=0, incl=[0, 2]), C.VALID_RESV_NODE, 0),
    ("included nodes inside the reservation", dict(p=0, tcpu=CORE, tmem=G, rsv=0, incl=[2]), C.VALID_OK, 1),
    ("a reservation job without lists walks the whole partition", dict(p=0, tcpu=CORE, tmem=G, rsv=0), C.VALID_OK, 4),
    ("n3 is shared by p0 and p1: 16 cores in p0", dict(p=0, tcpu=16 * CORE, tmem=G), C.VALID_OK, 2),
    ("... and in p1", dict(p=1, tcpu=16 * CORE, tmem=G), C.VALID_OK, 1),
]


def hand():
    """-> (cluster, reservations, jobs, expected code, expected eligible)"""
    cl = make_cluster(HAND_NODES, HAND_PARTS)
    return (cl, make_resv(cl, HAND_RESV), make_jobs([h[1] for h in HAND]), np.asarray([h[2] for h in HAND], np.uint8),
            np.asarray([h[3] for h in HAND], np.uint32))


# ---- the hand-derived table on wide GRES layouts (tests/gres_wide.py) --------------------------------------------------------------------
# The walk compares all classes (and all names) with one subtract-and-mask on packed bytes: a node byte is at most 64, a request byte is
# clamped to 65 (csrc/valid_kernels.inc, vd_fits).  These rows are decided by the clamp, by a byte's neighbour, by bit 63, by names 2 and
# 3 and class indices up to 7, and by partition sums that take more than one wave.  Every job: one core and 1 GiB per task, ntasks =
# node_num, on nodes of 8 cores and 16 GiB, so that only the GRES counts (and, in WIDE_MEM, the memory) decide.
M64 = 2 ** 64 - 1


def _w(p, k=1, gt=None, gs=None, **kw):
    return dict(p=p, tcpu=CORE, tmem=G, k=k, nt=k, gt=gt or {}, gs=gs or {}, **kw)


# one64: class 0 = name 0 = all 64 bits.
# p0 = {n0..n4: 64 slots, n5: 63 slots (bit 63 missing)}: 6 nodes, name 0 / class 0 total 5 * 64 + 63 = 383
# p1 = {n6..n262: 64 slots}: 257 nodes — one more than k_valid_totals's 256-thread stride —, total 257 * 64 = 16 448
WIDE_ONE64_NODES = [(8, 16 * G, M64, 1, 0)] * 5 + [(8, 16 * G, M64 >> 1, 1, 0)] + [(8, 16 * G, M64, 1, 0)] * 257
WIDE_ONE64_PARTS = [list(range(6)), list(range(6, 263))]
WIDE_ONE64 = [
    # untyped, one node: :7283 asks count * 1 <= 383, the walk asks count <= the node's 64 (63 on n5)
    ("untyped 63: every node", _w(0, gt={0: 63}), C.VALID_OK, 6),
    ("untyped 64: all but n5", _w(0, gt={0: 64}), C.VALID_OK, 5),
    ("untyped 65 <= 383 passes :7283; no node has 65", _w(0, gt={0: 65}), C.VALID_NOT_ENOUGH_NODES, 0),
    ("untyped 127 <= 383; decided by the clamp to 65", _w(0, gt={0: 127}), C.VALID_NOT_ENOUGH_NODES, 0),
    ("untyped 255 <= 383; decided by the clamp to 65", _w(0, gt={0: 255}), C.VALID_NOT_ENOUGH_NODES, 0),
    # typed (a total of 0 and class 0 specified): :7283 asks 0 <= 383 and count <= 383, the walk count <= the node's class 0
    ("typed 63", _w(0, gs={0: 63}), C.VALID_OK, 6),
    ("typed 64", _w(0, gs={0: 64}), C.VALID_OK, 5),
    ("typed 65", _w(0, gs={0: 65}), C.VALID_NOT_ENOUGH_NODES, 0),
    ("typed 127", _w(0, gs={0: 127}), C.VALID_NOT_ENOUGH_NODES, 0),
    ("typed 255", _w(0, gs={0: 255}), C.VALID_NOT_ENOUGH_NODES, 0),
    ("typed 64 under a total of 64", _w(0, gt={0: 64}, gs={0: 64}), C.VALID_OK, 5),
    ("typed 63 under a total of 64: the total decides n5", _w(0, gt={0: 64}, gs={0: 63}), C.VALID_OK, 5),
    # the same requests times a node_num that :7283 refuses (it comes before :7299's node_num > 6)
    ("63 * 6 = 378 <= 383: six nodes, six eligible", _w(0, k=6, gt={0: 63}), C.VALID_OK, 6),
    ("63 * 7 = 441 > 383", _w(0, k=7, gt={0: 63}), C.VALID_NO_RESOURCE, 0),
    ("64 * 5 = 320 <= 383: five nodes, five eligible", _w(0, k=5, gt={0: 64}), C.VALID_OK, 5),
    ("64 * 6 = 384 > 383: one slot short", _w(0, k=6, gt={0: 64}), C.VALID_NO_RESOURCE, 0),
    ("typed 64 * 6 = 384 > 383", _w(0, k=6, gs={0: 64}), C.VALID_NO_RESOURCE, 0),
    ("65 * 5 = 325 <= 383", _w(0, k=5, gt={0: 65}), C.VALID_NOT_ENOUGH_NODES, 0),
    ("65 * 6 = 390 > 383", _w(0, k=6, gt={0: 65}), C.VALID_NO_RESOURCE, 0),
    ("127 * 3 = 381 <= 383", _w(0, k=3, gs={0: 127}), C.VALID_NOT_ENOUGH_NODES, 0),
    ("127 * 4 = 508 > 383", _w(0, k=4, gs={0: 127}), C.VALID_NO_RESOURCE, 0),
    ("255 * 2 = 510 > 383", _w(0, k=2, gt={0: 255}), C.VALID_NO_RESOURCE, 0),
    # 257 nodes: the sums of k_valid_totals cross its stride, its waves and its LDS stage
    ("64 * 257 = 16 448 = the total: every node", _w(1, k=257, gt={0: 64}), C.VALID_OK, 257),
    ("typed 64 * 257 = 16 448", _w(1, k=257, gs={0: 64}), C.VALID_OK, 257),
    ("255 * 64 = 16 320 <= 16 448 passes :7283; no node has 255", _w(1, k=64, gt={0: 255}), C.VALID_NOT_ENOUGH_NODES, 0),
    ("255 * 65 = 16 575 > 16 448", _w(1, k=65, gt={0: 255}), C.VALID_NO_RESOURCE, 0),
    ("typed 255 * 64 = 16 320", _w(1, k=64, gs={0: 255}), C.VALID_NOT_ENOUGH_NODES, 0),
    ("typed 255 * 65 = 16 575", _w(1, k=65, gs={0: 255}), C.VALID_NO_RESOURCE, 0),
    ("65 * 253 = 16 445 <= 16 448", _w(1, k=253, gt={0: 65}), C.VALID_NOT_ENOUGH_NODES, 0),
    ("65 * 254 = 16 510 > 16 448", _w(1, k=254, gt={0: 65}), C.VALID_NO_RESOURCE, 0),
]


def _wide_eight():
    """eight_by_8_four_names: class_name [3, 0, 2, 1, 0, 3, 1, 2], 8 slots each; name 0 = classes 1, 4; name 1 = 3, 6; name 2 = 2, 7;
    name 3 = 0, 5.  n0, n1: every class full (8; every name 16).  n(2 + c): class c at 7 (its lowest slot missing), the others full, so
    the name of class c at 15.  One partition of the 10 nodes: every class sums to 9 * 8 + 7 = 79, every name to 158, far above any
    request here (:7283 passes everywhere)."""
    from tests import gres_wide as gw
    lay = gw.make_layout("eight_by_8_four_names")
    nodes = [(8, 16 * G, M64, 1, 0)] * 2 + [(8, 16 * G, M64 & ~(1 << lay.class_shift[c]), 1, 0) for c in range(8)]
    rows = []
    for c in range(8):
        nb = c + 1 if c < 7 else 6          # the class in the neighbouring byte of the packed word
        # 8 of class c: every node but n(2 + c)
        rows.append((f"class {c}: 8", _w(0, gs={c: 8}), C.VALID_OK, 9))
        # ... and 8 of the neighbour: every node but n(2 + c) and n(2 + nb)
        rows.append((f"class {c}: 8, and 8 of class {nb}", _w(0, gs={c: 8, nb: 8}), C.VALID_OK, 8))
        # 9 of class c: no node (the byte's own borrow), whatever the neighbour's byte says
        rows.append((f"class {c}: 9, and 8 of class {nb}", _w(0, gs={c: 9, nb: 8}), C.VALID_NOT_ENOUGH_NODES, 0))
    for a in range(4):
        nb = a + 1 if a < 3 else 2
        # 16 of name a: every node but the two with one of its classes at 7
        rows.append((f"name {a}: 16", _w(0, gt={a: 16}), C.VALID_OK, 8))
        # ... and 16 of the neighbour: but those four
        rows.append((f"name {a}: 16, and 16 of name {nb}", _w(0, gt={a: 16, nb: 16}), C.VALID_OK, 6))
        rows.append((f"name {a}: 17, and 16 of name {nb}", _w(0, gt={a: 17, nb: 16}), C.VALID_NOT_ENOUGH_NODES, 0))
        # 15 of name a, 8 of its first class: the node with that class at 7 has 15 of the name, but not the 8
        first = lay.class_name.index(a)
        rows.append((f"name {a}: 15 with 8 of its class {first}", _w(0, gt={a: 15}, gs={first: 8}), C.VALID_OK, 9))
    return lay, nodes, [list(range(10))], rows


# Three nodes of 2^63 bytes in one partition: 3 * 2^63 leaves 64 bits, the partition's sum saturates at UINT64_MAX (validity.h).
# 2^64 - 1 = 3 * 0x5555555555555555: three tasks of that much are a total of UINT64_MAX exactly and pass :7283 only against the saturated
# sum (a wrapped sum would be 2^63); each node holds one task (0x5555... <= 2^63).
WIDE_MEM_NODES = [(8, 1 << 63, 0, 1, 0)] * 3
WIDE_MEM = [
    ("total memory 2^64 - 1 against the saturated sum", dict(p=0, tcpu=CORE, tmem=0x5555555555555555, k=3, nt=3), C.VALID_OK, 3),
    ("one task of 2^63 on each node: 3 * 2^63 is not a 64-bit total", dict(p=0, tcpu=CORE, tmem=1 << 63, k=3, nt=3), C.VALID_BAD_REQUEST, 0),
    ("one task of 2^63: exactly a node's", dict(p=0, tcpu=CORE, tmem=1 << 63), C.VALID_OK, 3),
    ("one byte more than a node's, below the partition's", dict(p=0, tcpu=CORE, tmem=(1 << 63) + 1), C.VALID_NOT_ENOUGH_NODES, 0),
]


def hand_wide():
    """-> {table name: (cluster, jobs, expected code, expected eligible, rows)}"""
    from tests import gres_wide as gw
    lay8, nodes8, parts8, rows8 = _wide_eight()
    tables = {"one64": (make_cluster(WIDE_ONE64_NODES, WIDE_ONE64_PARTS, gw.make_layout("one64")), WIDE_ONE64),
              "eight_by_8_four_names": (make_cluster(nodes8, parts8, lay8), rows8),
              "mem_2pow63": (make_cluster(WIDE_MEM_NODES, [[0, 1, 2]]), WIDE_MEM)}
    return {name: (cl, make_jobs([r[1] for r in rows]), np.asarray([r[2] for r in rows], np.uint8), np.asarray([r[3] for r in rows], np.uint32), rows)
            for name, (cl, rows) in tables.items()}


# ---- the generator ---------------------------------------------------------------------------------------------------------------------
GPU_SEEDS = tuple(range(20))


def generate(seed: int):
    """A seeded cluster (3 or 4 partitions, some sharing nodes, <= 300 nodes from a small palette of records, mixed GRES, some nodes down,
    one partition with an unsupported node), reservations, and <= 500 jobs aimed at every code, with lists.  -> (cluster, resv, jobs)"""
    rng = np.random.default_rng(1000 + seed)
    N = int(rng.integers(40, 301))
    P = int(rng.integers(3, 5))
    palette = []
    for _ in range(int(rng.integers(4, 11))):
        cores = int(rng.choice([4, 8, 16, 32, 64]))
        mem = int(rng.choice([8, 16, 64, 256])) * G
        g = 0
        if rng.random() < 0.5:
            g |= (1 << int(rng.integers(0, 5))) - 1                   # a100 x 0..4
            g |= ((1 << int(rng.integers(0, 5))) - 1) << 4            # v100 x 0..4
        if rng.random() < 0.2:
            g |= ((1 << int(rng.integers(1, 3))) - 1) << 8            # fpga x 1..2
        palette.append((cores, mem, g))
    kind = rng.integers(0, len(palette), N)
    down = rng.random(N) < 0.15
    # A partition that shares a node with the unsupported one is refused by the cycle with it, and a snapshot the cycle refuses whole is
    # refused by cns_set_nodes.  So partition 0 is a clean range [0, cut) the cycle serves; partition 1 is a random subset
    # of [0, mid) that may overlap it; the others, the unsupported one among them, are random subsets of the rest that may overlap each other.
    cut = int(rng.integers(N // 4, N // 2))
    mid = cut + (N - cut) // 2
    parts = [list(range(cut))]
    for p in range(1, P):
        lo, hi = (0, mid) if p == 1 else (mid, N)
        size = int(rng.integers(1, max(2, (hi - lo) // 2 + 1)))
        parts.append(sorted(lo + int(x) for x in rng.choice(hi - lo, size, replace=False)))
    unsup = np.zeros(N, np.uint8)
    bad_part = P - 1
    cand = [n for n in parts[bad_part] if n >= cut]
    if cand:
        unsup[int(rng.choice(cand))] = 1
    refused = [any(unsup[n] for n in p) for p in parts]
    nodes = [(palette[kind[n]][0], palette[kind[n]][1], palette[kind[n]][2], 0 if down[n] else 1, int(unsup[n])) for n in range(N)]
    cl = make_cluster(nodes, parts)
    V = int(rng.integers(1, 4))
    resv_lists = [sorted(int(x) for x in rng.choice(N, int(rng.integers(1, 20)), replace=False)) for _ in range(V)]
    resv = make_resv(cl, resv_lists)

    good = [p for p in range(P) if not refused[p]]
    J = int(rng.integers(250, 501))
    rows = []
    targets = ["ok"] * 4 + ["bad", "zmem", "zcpu", "nopart", "refused", "nores", "nodenum", "norsv", "rsvnode", "few", "few"]
    for _ in range(J):
        t = targets[int(rng.integers(0, len(targets)))]
        p = int(rng.choice(good))
        pn = parts[p]
        r = dict(p=p, tcpu=int(rng.choice([1, 2, 4])) * CORE, tmem=int(rng.choice([1, 2, 4])) * G, k=1, nt=1)
        if rng.random() < 0.3:
            r["k"] = int(rng.integers(1, min(len(pn), 6) + 1))
            r["nt"] = r["k"] * int(rng.integers(1, 3))
        if rng.random() < 0.25:
            r["gt"] = {GPU: int(rng.integers(1, 4))}
        if rng.random() < 0.15:
            r["gs"] = {int(rng.integers(0, 2)): int(rng.integers(1, 3))}
        lists = rng.random()
        if lists < 0.12:
            r["incl"] = [int(x) for x in rng.choice(N + 5, int(rng.integers(1, 12)), replace=False)]
        elif lists < 0.24:
            r["excl"] = [int(x) for x in rng.choice(N + 5, int(rng.integers(1, 30)), replace=False)]
        elif lists < 0.28:
            r["incl"] = [int(x) for x in rng.choice(pn, min(len(pn), int(rng.integers(1, 8))), replace=False)]
            r["excl"] = [int(x) for x in rng.choice(N, int(rng.integers(1, 10)), replace=False)]
        if rng.random() < 0.1:
            r["rsv"] = int(rng.integers(0, V))
        if t == "bad":
            w = int(rng.integers(0, 3))
            if w == 0:
                r["k"] = 0
            elif w == 1:
                r["k"], r["nt"] = 3, 2
            else:
                r["tmem"], r["nt"] = 1 << 62, max(4, r["nt"])
        elif t == "zmem":
            r["tmem"] = 0
        elif t == "zcpu":
            r["tcpu"] = 0
        elif t == "nopart":
            r["p"] = P + int(rng.integers(0, 3))
        elif t == "refused":
            r["p"] = bad_part
        elif t == "nores":
            w = int(rng.integers(0, 3))
            if w == 0:
                r["tmem"] = 1 << 50
            elif w == 1:
                r["gs"] = {int(rng.integers(3, 8)): 1}
            else:
                r["gt"] = {int(rng.integers(2, 4)): 1}
        elif t == "nodenum":
            r.update(k=len(pn) + int(rng.integers(1, 4)), tcpu=CORE, tmem=G)
            r["nt"] = r["k"]
            r.pop("gt", None), r.pop("gs", None)
        elif t == "norsv":
            r["rsv"] = V + int(rng.integers(0, 3))
        elif t == "rsvnode":
            r["rsv"] = int(rng.integers(0, V))
            outside = [n for n in range(N) if n not in resv_lists[r["rsv"]]]
            r["incl"] = [int(rng.choice(outside))] + resv_lists[r["rsv"]][:2]
            r.pop("excl", None)
        elif t == "few":
            w = int(rng.integers(0, 3))
            if w == 0:
                r.update(tcpu=64 * CORE, k=min(len(pn), 4), nt=min(len(pn), 4))
            elif w == 1:
                r["excl"] = list(pn)
                r.pop("incl", None)
            else:
                r["incl"] = [int(rng.choice(pn))]
                r.pop("excl", None)
                r.update(k=min(len(pn), 2), nt=2)
        rows.append(r)
    return cl, resv, make_jobs(rows)


@functools.lru_cache(maxsize=None)
def generated(seed: int):
    """generate(seed) with the truth's answer, computed once per process: -> (cluster, resv, jobs, code, eligible)"""
    from tests import valid_pyref
    cl, resv, jobs = generate(seed)
    code, elig = valid_pyref.check(cl, jobs, valid_pyref.resv_node_sets(resv))
    return cl, resv, jobs, code, elig
