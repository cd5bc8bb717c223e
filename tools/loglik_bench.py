#!/usr/bin/env python3
"""Cost of the pointwise log-likelihood draws (dcfm_set_loglik) at the bench shape c3 (p = 19,968, g = 64,
K = 30, n = 1,000) by default, on a handle set up the way bench.py sets one up (synthetic sparse-factor data,
on-device ingest and initial state).  Prints one JSON line.  The c4 shape is --g 8 --P 1250 --K 100 --n 2000.

--mode save        thin = 1, so every iteration saves a sample; only DCFM_K_SAVE is timed (HIP events around the
                   save and everything launched behind it).  Runs of --iters iterations alternate the feature off /
                   on --repeats times after --warmup pairs; the medians' difference is the whole launch chain's
                   device time per saved sample.  (K <= 32, feature off: k_lambda saves and nothing is timed, 0.)
--mode throughput  the bench's settings (--thin 5, --iters 480, asm_batch 96): wall time of run + synchronize,
                   interleaved off / on pairs on one handle; iterations per second of each and the ratio.
--mode kernels     one run of --iters iterations, thin = 1, feature on, DCFM_FLAG_UNFUSED, DCFM_K_WPASS and
                   DCFM_K_SAVE timed: the unfused k_wpass per launch beside the save chain; run it under a kernel
                   trace (rocprofv3 --kernel-trace --stats -- python tools/loglik_bench.py --mode kernels) for
                   the per-kernel times of k_loglik_ypass, k_precision, k_loglik_sinv and k_loglik_close."""
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
    ap.add_argument("--mode", choices=("save", "throughput", "kernels"), default="save")
    ap.add_argument("--g", type=int, default=64)
    ap.add_argument("--P", type=int, default=312)
    ap.add_argument("--n", type=int, default=1000)
    ap.add_argument("--K", type=int, default=30)
    ap.add_argument("--thin", type=int, default=None)
    ap.add_argument("--iters", type=int, default=None)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()

    import __graft_entry__ as ge
    from bench import synth_data
    dcfm = ge.load_package()
    from dcfm_amd import _abi
    g, P, n, K = args.g, args.P, args.n, args.K
    p = g * P
    thin = args.thin or (5 if args.mode == "throughput" else 1)
    iters = args.iters or {"save": 100, "throughput": 480, "kernels": 40}[args.mode]
    Y = synth_data(n, p)
    Y = Y[0] if isinstance(Y, tuple) else Y
    keep = np.flatnonzero(dcfm.count_nonzero_columns(Y) != 0)
    assert keep.size == p, "synthetic data has an all-zero column"
    init = dcfm.driver._HostVarind(1, p)
    rounds = 1 if args.mode == "kernels" else args.warmup + args.repeats
    smp = dcfm.Sampler(n, P, g, K, 0.5, 0, 2 * rounds * iters, thin, seed=1,
                       asm_batch=96 if args.mode == "throughput" else 0,
                       flags=_abi.DCFM_FLAG_UNFUSED if args.mode == "kernels" else 0)
    out = {"mode": args.mode, "p": p, "g": g, "P": P, "K": K, "n": n, "thin": thin, "iters_per_run": iters}
    first = 1
    try:
        smp.set_data_raw(Y, dcfm.shard_columns(keep, init.varind, P, 0, g))
        smp.init_state()
        if args.mode == "kernels":
            smp.set_loglik(iters)
            smp.set_profiling_kernels(["k_wpass", "k_save"])
            smp.run(1, iters)
            smp.synchronize()
            st = smp.kernel_stats()
            out.update({k + "_us_per_launch": round(st[k][0] / max(st[k][1], 1) * 1e3, 3) for k in ("k_wpass", "k_save")})
            assert smp.loglik_draws().shape == (iters, n)
        else:
            res = {"off": [], "on": []}
            for r in range(rounds):
                for mode in ("off", "on"):
                    smp.set_loglik(iters // thin + 1 if mode == "on" else 0)
                    if args.mode == "save":
                        smp.set_profiling_kernels(["k_save"])
                    smp.synchronize()
                    t0 = time.perf_counter()
                    smp.run(first, iters)
                    smp.synchronize()
                    dt = time.perf_counter() - t0
                    first += iters
                    if args.mode == "save":
                        ms, cnt = smp.kernel_stats()["k_save"]
                        val = round(ms / cnt * 1e3, 3) if cnt else 0.0
                    else:
                        val = round(iters / dt, 2)
                    if r >= args.warmup:
                        res[mode].append(val)
            off, on = statistics.median(res["off"]), statistics.median(res["on"])
            if args.mode == "save":
                out.update({"k_save_us_per_launch": res, "median_off_us": off, "median_on_us": on,
                            "loglik_us_per_saved_sample": round(on - off, 3)})
            else:
                out.update({"iters_per_s": res, "median_off": off, "median_on": on, "on_over_off": round(on / off, 4)})
    finally:
        smp.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
