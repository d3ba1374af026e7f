"""cns_running_amend_ends against the only way a caller had before it: cns_running_seed of the whole amended running set.  Scale C4r
(65 536 nodes, 300 000 running jobs drawn, cranesched_amd/synth.py).  K = 1 and K = 1 000 running jobs get a new end; in one process,
alternating per repetition:
  (a) cns_running_amend_ends on the handle that holds the ledger: the K ids and ends go up, the end column and the per-slot end times
      are rewritten on the device;
  (b) cns_running_seed of the same amended set on a second handle: every allocation goes up, is expanded and sorted again.
Two warm-up repetitions, then --reps (at least 20).  Host clock around each synchronous call through the Python binding; the HIP-event
split as the engine reports it (cns_running_amend_get_timing, cns_running_get_timing).  Asserted in the run: after every repetition the
two ledgers hold the same ends, and at the end a cycle on either handle gives the same placements and fp64 cost bits.
Prints one JSON line.

usage: python tools/running_amend_bench.py [--reps 20] [--small]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cranesched_amd import synth  # noqa: E402
from cranesched_amd.engine import GpuNodeSelector  # noqa: E402


def clock(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t0) * 1e3


def stats(v):
    return {"median": round(float(np.median(v)), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--small", action="store_true", help="C4r scaled to 4 096 nodes")
    a = ap.parse_args()
    reps = max(a.reps, 20)
    cluster, jobs, now, run = synth.make_loaded("C4r", J=2000, N=4096 if a.small else None)
    R = len(run.end_sec)
    ids = (1 + np.arange(R)).astype(np.uint32)
    amend, seed = GpuNodeSelector(device=0), GpuNodeSelector(device=0)
    amend.set_nodes(cluster)
    seed.set_nodes(cluster)
    amend.seed_running(run, ids)
    rng = np.random.default_rng(26)
    out = {"shape": {"nodes": cluster.num_nodes, "running": R, "allocations": int(run.alloc_offsets[-1])}, "reps": reps}
    for K in (1, 1000):
        rows = {k: [] for k in ("amend_ms", "amend_h2d_ms", "amend_kernels_ms", "amend_d2h_ms", "seed_ms", "seed_h2d_ms", "seed_kernels_ms", "seed_d2h_ms")}
        for rep in range(reps + 2):
            pick = rng.choice(R, K, replace=False)
            new = now + 60 * rng.integers(1, 600, K)
            (found, n), t_am = clock(lambda: amend.amend_running(ids[pick], new))
            ta = amend.running_amend_timing()
            assert n == K and found.all() and ta["rows"] == R and ta["pairs"] > 0
            run.end_sec[pick] = new
            _, t_seed = clock(lambda: seed.seed_running(run, ids))
            ts = seed.running_timing()
            assert ts["pairs"] == ta["pairs"]
            if rep >= 2:
                for k, v in (("amend_ms", t_am), ("amend_h2d_ms", ta["h2d_ms"]), ("amend_kernels_ms", ta["kernels_ms"]), ("amend_d2h_ms", ta["d2h_ms"]),
                             ("seed_ms", t_seed), ("seed_h2d_ms", ts["h2d_ms"]), ("seed_kernels_ms", ts["kernels_ms"]), ("seed_d2h_ms", ts["d2h_ms"])):
                    rows[k].append(v)
        assert np.array_equal(amend.running_ledger()[0].end_sec, run.end_sec), "the amended ledger is not the set that was seeded"
        out[f"K={K}"] = {k: stats(v) for k, v in rows.items()}
        out[f"K={K}"]["pairs"] = int(ta["pairs"])
    pa, ps = amend.node_select(now, jobs), seed.node_select(now, jobs)
    assert pa.diff(ps) is None and np.array_equal(amend.costs().view(np.uint64), seed.costs().view(np.uint64)), "a cycle differs between the two handles"
    out["cycles_equal"] = True
    print(json.dumps(out))
    amend.close()
    seed.close()


if __name__ == "__main__":
    main()
