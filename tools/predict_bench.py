#!/usr/bin/env python3
"""Cost of the conditional prediction (dcfm_set_predict) per saved sample, at the bench shape c3
(p = 19,968, g = 64, K = 30) by default, on a handle set up the way bench.py sets one up (synthetic
sparse-factor data, on-device ingest and initial state).  thin = 1, so every iteration saves a sample; only
DCFM_K_SAVE is timed (HIP events around k_save, and k_precision, k_predict_coef and k_predict_apply behind it
when the feature is on).  Runs of --iters iterations alternate the feature off / on (nt = --nt seeded normal new
rows under a seeded mask with a fraction --observed of the variables observed; 0: the variances and the log det
alone) --repeats times after --warmup pairs; prints one JSON line with the per-launch device time of
DCFM_K_SAVE of every run, the medians and their difference: the feature's device time per saved sample.
--yardstick runs the precision probes at nv = nt instead (tools/precision_bench.py's measurement, in the same
session).  The c4 shape is --g 8 --P 1250 --K 100 --n 2000."""
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
    ap.add_argument("--nt", type=int, default=32)
    ap.add_argument("--observed", type=float, default=0.6)
    ap.add_argument("--yardstick", action="store_true")
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
    rng = np.random.default_rng(0)
    V = rng.standard_normal((p, args.nt))
    obs = rng.random(p) < args.observed
    us = {"off": [], "on": []}
    first = 1
    try:
        smp.set_data_raw(Y, dcfm.shard_columns(keep, init.varind, P, 0, g))
        smp.init_state()
        for r in range(rounds):
            for mode in ("off", "on"):
                if args.yardstick:
                    smp.set_precision_probes(V if mode == "on" else None, args.iters)
                elif mode == "on":
                    smp.set_predict(V, obs, args.iters)
                else:
                    smp.set_predict(None, None, 0)
                smp.set_profiling_kernels(["k_save"])
                smp.run(first, args.iters)
                smp.synchronize()
                first += args.iters
                ms, cnt = smp.kernel_stats()["k_save"]
                held = smp.precision_draws()[1].shape[0] if args.yardstick else smp.predict_raw()[5]
                # feature off at K <= 32: k_lambda saves the sample itself and nothing is booked under DCFM_K_SAVE
                assert cnt in ((args.iters,) if mode == "on" else (0, args.iters)), cnt
                assert held == (args.iters if mode == "on" else 0)
                if r >= args.warmup:
                    us[mode].append(round(ms / cnt * 1e3, 3) if cnt else 0.0)
    finally:
        smp.close()
    off, on = statistics.median(us["off"]), statistics.median(us["on"])
    print(json.dumps({"p": p, "g": g, "P": P, "K": K, "n": n, "nt": args.nt, "observed": args.observed,
                      "what": "precision_probes" if args.yardstick else "predict", "iters_per_run": args.iters,
                      "k_save_us_per_launch": us, "median_off_us": off, "median_on_us": on,
                      "feature_us_per_saved_sample": round(on - off, 3)}))


if __name__ == "__main__":
    main()
