"""A model of k_giant and k_mem at giant widths (wide_kernel.inc: giant_helper / giant_scan, mem_scan_serial / margmin; the giant
instantiation k_wide<1, false, kWMemWordsGiant>, launch_giant / launch_mem).  Round 0 of each phase comes from the helper workgroups'
stripes (lane gl = h * 512 + t owns slots rb + gl + i * 512 nh), reduced by the home; every later step from the home's masks.
Constants are read from the engine's source.

Each of the 448 memory-scanner lanes owns a stripe of the job's slot range [rb, rb + rn): row r of lane ml is slot rb + r * 448 + ml,
one bit per row in MW 64-bit words of each mask (start-now set A, res_total set B, used).  Per step of the walk every lane answers with
its stripe's lexicographic (cost key, slot) minimum over mask & ~used, and the workgroup reduces the 448 answers.  Here, on random rows
with cost ties, empty stripes, own-partition ranges of a group, include / exclude lists and Phase A -> Phase B fall-through, the reduced
answers must give the same walk, step for step, as ONE scanner that sorts the eligible slots by (cost key, slot) — the order of
GetNodesAndTrySchedule_'s loop (tests/select_pyref.py, Cycle.try_schedule).  And the row masks must hold every width the host admits:
the ordinary 5 words up to 143 360 slots, the giant 19 words up to 524 288."""
import os
import re

import numpy as np
import pytest

_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cranesched_amd", "csrc")


def _const(fname, name):
    """A constexpr of the engine's source (so that the model follows the kernel's constants)."""
    src = open(os.path.join(_CSRC, fname)).read()
    m = re.search(r"constexpr u32 " + name + r" = (\d+)", src)
    assert m, name
    return int(m.group(1))


LANES = 7 * 64          # kWMs: the seven tester waves of the home workgroup (kWBlock / 64 - 1 waves of 64 lanes)
MW_ORDINARY, MW_GIANT = _const("wide_kernel.inc", "kWMemWords"), _const("wide_kernel.inc", "kWMemWordsGiant")
MEM_SLOTS, GIANT_MEM_SLOTS = LANES * 64 * MW_ORDINARY, LANES * 64 * MW_GIANT
GIANT_PART, GIANT_GROUP = _const("engine.hip", "kGiantPartSlots"), _const("engine.hip", "kGiantGroupSlots")
HELPERS = min(_const("wide_kernel.inc", "kGiantHelpersMax"), _const("engine.hip", "kGiantHelperBudget"))
HELPER_LANES = 512      # kWBlock: lanes of one helper workgroup


def words_needed(rn):
    rows = (rn + LANES - 1) // LANES
    return (rows + 63) // 64


class StripedScanner:
    """The lanes' masks as k_mem keeps them: bit r of word r >> 6 of lane ml <-> slot rb + r * LANES + ml."""

    def __init__(self, rb, rn, mw):
        self.rb, self.rn, self.mw = rb, rn, mw
        self.rows = (rn + LANES - 1) // LANES
        assert (self.rows + 63) // 64 <= mw, "row masks too narrow for the range"
        self.masks = {k: np.zeros((LANES, mw), np.uint64) for k in ("a", "b", "used")}

    def slot(self, ml, r):
        return self.rb + r * LANES + ml

    def set_bits(self, name, slots):
        m = self.masks[name]
        for p in slots:
            off = p - self.rb
            ml, r = off % LANES, off // LANES
            m[ml, r >> 6] |= np.uint64(1) << np.uint64(r & 63)

    def clear_used(self):
        self.masks["used"][:] = 0

    def lane_argmin(self, ml, name, key):
        """margmin: the lane's (cost key, slot) minimum over mask & ~used (ascending rows, strict <)."""
        best = (None, None)
        for w in range(self.mw):
            m = int(self.masks[name][ml, w]) & ~int(self.masks["used"][ml, w]) & ((1 << 64) - 1)
            while m:
                r = w * 64 + ((m & -m).bit_length() - 1)
                m &= m - 1
                p = self.slot(ml, r)
                if best[0] is None or key[p] < best[0]:
                    best = (key[p], p)
        return best

    def step(self, name, key):
        """Every lane's answer, reduced (reduce16: smallest key, then smallest slot)."""
        answers = [self.lane_argmin(ml, name, key) for ml in range(LANES)]
        live = [a for a in answers if a[0] is not None]
        return min(live) if live else (None, None)

    def mark_used(self, p):
        self.set_bits("used", [p])


def helper_round0(rb, rn, slots, key, nh):
    """k_giant's round 0: helper h, lane t owns slots rb + gl, rb + gl + stride, ... (gl = h * 512 + t, stride = nh * 512); each helper
    answers its stripe's (cost key, slot) minimum (giant_scan: ascending slots, strict <), the home reduces the nh answers."""
    stride = nh * HELPER_LANES
    answers = []
    for h in range(nh):
        lanes = []
        for t in range(HELPER_LANES):
            best = (None, None)
            for p in slots.get(h * HELPER_LANES + t, ()):   # (the slots of this lane's stripe, ascending: strict < keeps the first)
                if best[0] is None or key[p] < best[0]:
                    best = (key[p], p)
            if best[0] is not None:
                lanes.append(best)
        answers.append(min(lanes) if lanes else (None, None))   # wave_argmin + reduce16: lexicographic (key, slot)
    live = [a for a in answers if a[0] is not None]
    return min(live) if live else (None, None)


def walk_striped(sc, key, visit_a, visit_b, helpers=None):
    """Phase A over the start-now set, then Phase B over the res_total set with `used` cleared (:6335 ff.); visit_x(slot) -> True ends
    the phase's walk (the verdict / the k-th node / the tasks are covered).  helpers: {"a": set, "b": set} -> round 0 of each phase from
    the helpers' stripes (k_giant), every later step from the home's masks (built on demand)."""
    seq = []
    for name, visit in (("a", visit_a), ("b", visit_b)):
        sc.clear_used()
        first = True
        while True:
            if first and helpers is not None:
                by_lane = {}
                for p in sorted(helpers[name]):
                    by_lane.setdefault((p - sc.rb) % (HELPERS * HELPER_LANES), []).append(p)
                _, p = helper_round0(sc.rb, sc.rn, by_lane, key, HELPERS)
            else:
                _, p = sc.step(name, key)
            first = False
            if p is None:
                break
            seq.append((name, p))
            sc.mark_used(p)
            if visit(p):
                return seq
    return seq


def walk_single(slots_a, slots_b, key, visit_a, visit_b):
    seq = []
    for name, slots, visit in (("a", slots_a, visit_a), ("b", slots_b, visit_b)):
        for p in sorted(slots, key=lambda x: (key[x], x)):
            seq.append((name, p))
            if visit(p):
                return seq
    return seq


def _case(rng, width, rb, rn, exclusive, lists):
    """Random rows over [rb, rb + rn) of a group of `width` slots: costs from a small set (many ties), B = res_total fits, A = start now
    (a subset of B; exclusive jobs: only completely free nodes), then the include / exclude lists."""
    key = rng.choice(np.array([0, 1 << 52, 3 << 50, 1 << 60], np.uint64), width)   # fp64 cost keys: few values, many ties
    own = np.arange(rb, rb + rn)
    b = own[rng.random(rn) < rng.choice([0.0, 0.002, 0.02, 0.3])]
    free = rng.random(len(b)) < (0.2 if exclusive else 0.6)
    a = b[free]
    if lists:
        incl = set(rng.choice(own, min(rn, 500), replace=False).tolist())
        excl = set(rng.choice(own, min(rn, 50), replace=False).tolist())
        a = np.array([p for p in a if p in incl and p not in excl], np.int64)
        b = np.array([p for p in b if p in incl and p not in excl], np.int64)
    return key, a, b


@pytest.mark.parametrize("seed", range(6))
def test_striped_walk_matches_one_scanner(seed):
    rng = np.random.default_rng(seed)
    layouts = [(GIANT_PART, 0, GIANT_PART),                               # one partition at the limit
               (GIANT_GROUP, GIANT_PART, GIANT_PART),                     # the second member of ALL + subsets
               (GIANT_GROUP, 1000, GIANT_GROUP - 1000 - 7),               # an own range that starts and ends off a stripe boundary
               (MEM_SLOTS + 1, 0, MEM_SLOTS + 1)]                         # one slot beyond the ordinary masks
    for width, rb, rn in layouts:
        for exclusive, lists in ((False, False), (True, False), (False, True)):
            key, a, b = _case(rng, width, rb, rn, exclusive, lists)
            sc = StripedScanner(rb, rn, MW_GIANT)
            sc.set_bits("a", a.tolist())
            sc.set_bits("b", b.tolist())
            # Phase A: the exact test fails on a random subset (the walk goes on), Phase B: k nodes, or ntasks > node_num (tasks summed)
            fail_a = set(rng.choice(a, min(len(a), 3), replace=False).tolist()) if len(a) else set()
            k = int(rng.integers(1, 5))
            tasks = {p: int(rng.integers(1, 3)) for p in b.tolist()}
            general = bool(rng.integers(0, 2))
            state = {"n": 0, "t": 0}

            def visit_a(p):
                return p not in fail_a

            def visit_b(p):
                state["n"] += 1
                state["t"] += tasks[p]
                return state["t"] >= k + 1 if general else state["n"] == k

            got = walk_striped(sc, key, visit_a, visit_b, None if lists else {"a": set(a.tolist()), "b": set(b.tolist())})
            state.update(n=0, t=0)
            want = walk_single(a.tolist(), b.tolist(), key, visit_a, visit_b)
            assert got == want, (width, rb, rn, exclusive, lists)


def test_every_admitted_width_fits_the_masks():
    """The host's limits against the masks: what k_mem's ordinary instantiation serves fits 5 words, the giant one 19 words; the widest group
    the host admits (524 288 slots) fits the giant masks, one slot more would not fit the ordinary ones."""
    assert words_needed(MEM_SLOTS) <= MW_ORDINARY < words_needed(MEM_SLOTS + 1)
    assert words_needed(GIANT_GROUP) <= MW_GIANT and words_needed(GIANT_PART) <= MW_GIANT
    assert GIANT_MEM_SLOTS >= GIANT_GROUP
    for rn in (1, LANES - 1, LANES, LANES + 1, 65_536, 143_360, 143_361, 262_144, 524_288):
        assert words_needed(rn) <= MW_GIANT


def test_empty_stripes_and_a_single_slot():
    """Most lanes with nothing to offer (a set of one slot, or none): the reduction skips them."""
    key = np.zeros(GIANT_PART, np.uint64)
    sc = StripedScanner(0, GIANT_PART, MW_GIANT)
    assert sc.step("a", key) == (None, None)
    sc.set_bits("a", [GIANT_PART - 1])
    assert sc.step("a", key) == (0, GIANT_PART - 1)
    sc.mark_used(GIANT_PART - 1)
    assert sc.step("a", key) == (None, None)
