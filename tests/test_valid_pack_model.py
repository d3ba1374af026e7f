"""A CPU model of the walk kernel's packed comparison (csrc/valid_kernels.inc: vd_fits on the class bytes of one 64-bit word and the name
bytes of one 32-bit word, request bytes clamped to 65) against the restatement's operator<=(ResourceView, ResourceInNodeV3): the
subtract-and-mask says "fits" exactly where PublicHeader.cpp:619-646 does, for every count a byte can carry."""
import numpy as np

from cranesched_amd import abi
from tests import valid_case as vc
from tests import valid_pyref as ref

HIGH64, HIGH32 = 0x8080808080808080, 0x80808080
# eight classes of eight slots each over four names: every byte of both words is in use, 64 slots in all
LAYOUT = abi.GresLayout(class_name=[0, 0, 0, 1, 1, 2, 3, 3], class_shift=[8 * c for c in range(8)], class_width=[8] * 8)


def pack_node(layout, mask):
    cls = names = 0
    for c in range(len(layout.class_name)):
        cnt = bin(mask & layout.class_mask(c)).count("1")
        cls |= cnt << (8 * c)
        names += cnt << (8 * layout.class_name[c])     # (a name's total is at most 64: no carry into the next byte)
    return cls, names


def fits(spec, tot, cls, names):
    need_c = sum(min(spec[c], 65) << (8 * c) for c in range(8))
    need_n = sum(min(tot[k], 65) << (8 * k) for k in range(4))
    return ((((cls | HIGH64) - need_c) & HIGH64) == HIGH64) and ((((names | HIGH32) - need_n) & HIGH32) == HIGH32)


def test_packed_comparison_equals_the_restatement():
    rng = np.random.default_rng(5)
    masks = [0, 2 ** 64 - 1, 0xFF, 0xFF << 56] + [int(rng.integers(0, 2 ** 63)) * 2 + int(rng.integers(0, 2)) for _ in range(60)]
    nodes = [(4, vc.G, m, 1, 0) for m in masks]
    cl = vc.make_cluster(nodes, [list(range(len(nodes)))], layout=LAYOUT)
    rows = []
    for _ in range(400):
        r = dict(p=0, tcpu=vc.CORE, tmem=vc.G, gt={}, gs={})
        for k in range(4):
            if rng.random() < 0.3:
                r["gt"][k] = int(rng.choice([1, 2, 8, 9, 16, 17, 24, 64, 65, 66, 128, 255]))
        for c in range(8):
            if rng.random() < 0.12:
                r["gs"][c] = int(rng.choice([1, 2, 7, 8, 9, 64, 65, 127, 128, 255]))
        rows.append(r)
    jobs = vc.make_jobs(rows)
    agree = pairs = 0
    for j in range(jobs.num_jobs):
        g = ref.job_gres(cl, jobs, j)
        for n in range(cl.num_nodes):
            want = ref.view_le_node((vc.CORE, vc.G, g), 4 * vc.CORE, vc.G, ref.node_gres(cl, n))
            got = fits([int(x) for x in jobs.gres_spec[j]], [int(x) for x in jobs.gres_total[j]], *pack_node(LAYOUT, int(cl.gres_slots[n])))
            assert got == want, (rows[j], hex(int(cl.gres_slots[n])))
            agree += want
            pairs += 1
    assert 0.02 * pairs <= agree <= 0.98 * pairs, "the draw exercises both answers"
