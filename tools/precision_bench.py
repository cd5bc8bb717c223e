#!/usr/bin/env python3
"""Cost of the precision draws (dcfm_set_precision_probes) per saved sample, at the bench shape c3
(p = 19,968, g = 64, K = 30) by default, on a handle set up the way bench.py sets one up (synthetic
sparse-factor data, on-device ingest and initial state).  thin = 1, so every iteration saves a sample; only
DCFM_K_SAVE is timed (HIP events around k_save, and k_precision behind it when the feature is on).  Runs of
--iters iterations alternate the feature off / on (nv = --nv seeded normal probes; 0: the log det alone)
--repeats times after --warmup pairs; prints one JSON line with the per-launch device time of DCFM_K_SAVE
of every run, the medians and their difference: the feature's device time per saved sample.  The c4 shape
is --g 8 --P 1250 --K 100 --n 2000."""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--g", type=int, default=64)
    ap.add_argument("--P", type=int, default=312)
    ap.add_argument("--n", type=int, default=1000)
    ap.add_argument("--K", type=int, default=30)
    ap.add_argument("--nv", type=int, default=32)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()

    import __graft_entry__ as ge
    from bench import synth_data
    dcfm = ge.load_package()
    g, P, n, K = args.g, args.P, args.n, args.K
    p = g * P
    Y = synth_data(n, p)
    Y = Y[0] if isinstance(Y, tuple) else Y
    keep = np.flatnonzero(dcfm.count_nonzero_columns(Y) != 0)
    assert keep.size == p, "synthetic data has an all-zero column"
    init = dcfm.driver._HostVarind(1, p)
    rounds = args.warmup + args.repeats
    smp = dcfm.Sampler(n, P, g, K, 0.5, 0, 2 * rounds * args.iters, 1, seed=1)
    V = np.random.default_rng(0).standard_normal((p, args.nv))
    us = {"off": [], "on": []}
    first = 1
    try:
        smp.set_data_raw(Y, dcfm.shard_columns(keep, init.varind, P, 0, g))
        smp.init_state()
        for r in range(rounds):
            for mode in ("off", "on"):
                smp.set_precision_probes(V if mode == "on" else None, args.iters)
                smp.set_profiling_kernels(["k_save"])
                smp.run(first, args.iters)
                smp.synchronize()
                first += args.iters
                ms, cnt = smp.kernel_stats()["k_save"]
                assert cnt == args.iters and smp.precision_draws()[1].shape[0] == (args.iters if mode == "on" else 0)
                if r >= args.warmup:
                    us[mode].append(round(ms / cnt * 1e3, 3))
    finally:
        smp.close()
    off, on = statistics.median(us["off"]), statistics.median(us["on"])
    print(json.dumps({"p": p, "g": g, "P": P, "K": K, "n": n, "nv": args.nv, "iters_per_run": args.iters,
                      "k_save_us_per_launch": us, "median_off_us": off, "median_on_us": on,
                      "precision_us_per_saved_sample": round(on - off, 3)}))


if __name__ == "__main__":
    main()
