#!/usr/bin/env python3
"""Cost of the imputation step (dcfm_set_missing) per Gibbs iteration, at the bench shape c3 (p = 19,968, g = 64,
K = 30) by default, on a handle set up the way bench.py sets one up (synthetic sparse-factor data, on-device
ingest and initial state, thin = 5).  For every missing rate of --rates (completely at random, seeded) runs of
--iters iterations alternate the feature off / on, --repeats times after --warmup pairs; each mode runs twice:
once unprofiled for the wall-clock throughput (iterations per second of dcfm_run + synchronize) and once with
DCFM_K_SAVE alone timed by HIP events, whose difference on - off over the iterations is the step's device time
per iteration (k_impute + k_impute_yy; at K > 32 the scope also holds k_save on the saved iterations, in both
modes).  Prints one JSON line per rate.  The c4 shape is --g 8 --P 1250 --K 100 --n 2000."""
import argparse
import json
import statistics
import sys
import time
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
    ap.add_argument("--thin", type=int, default=5)
    ap.add_argument("--rates", type=float, nargs="+", default=[0.01, 0.05, 0.20])
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
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
    total = 4 * rounds * args.iters * len(args.rates)
    smp = dcfm.Sampler(n, P, g, K, 0.5, 0, total, args.thin, seed=1)
    first = 1
    try:
        smp.set_data_raw(Y, dcfm.shard_columns(keep, init.varind, P, 0, g))
        smp.init_state()
        for rate in args.rates:
            mask = np.random.default_rng(7).random((n, P, g)) < rate
            us, ips, set_s = {"off": [], "on": []}, {"off": [], "on": []}, []
            for r in range(rounds):
                for mode in ("off", "on"):
                    t0 = time.perf_counter()
                    smp.set_missing(mask if mode == "on" else None, args.iters)
                    if mode == "on":
                        set_s.append(round(time.perf_counter() - t0, 3))
                    for profiled in (False, True):
                        smp.set_profiling_kernels(["k_save"] if profiled else [])
                        t0 = time.perf_counter()
                        smp.run(first, args.iters)
                        smp.synchronize()
                        dt = time.perf_counter() - t0
                        first += args.iters
                        if r < args.warmup:
                            continue
                        if profiled:
                            us[mode].append(round(smp.kernel_stats()["k_save"][0] / args.iters * 1e3, 3))
                        else:
                            ips[mode].append(round(args.iters / dt, 1))
            off, on = statistics.median(us["off"]), statistics.median(us["on"])
            ioff, ion = statistics.median(ips["off"]), statistics.median(ips["on"])
            print(json.dumps({"p": p, "g": g, "P": P, "K": K, "n": n, "thin": args.thin, "rate": rate,
                              "missing": int(mask.sum()), "iters_per_run": args.iters,
                              "k_save_us_per_iteration": us, "step_us_per_iteration": round(on - off, 3),
                              "iters_per_s": ips, "median_iters_per_s_off": ioff, "median_iters_per_s_on": ion,
                              "throughput_on_over_off": round(ion / ioff, 4), "set_missing_s": set_s}), flush=True)
    finally:
        smp.close()


if __name__ == "__main__":
    main()
