#!/usr/bin/env python3
"""Flushes of the regression stage (DCFM_FLAG_REGRESSION, dcfm_set_regression) at the bench shape c3 (p = 19,968,
g = 64, K = 30, thin 5, the library's default asm_batch of 32 samples per flush) by default, on a handle set up
the way bench.py sets one up (synthetic sparse-factor data, on-device ingest and initial state), with --q
responses spread over the shards.  The per-kernel times (k_reg_small, k_reg_rows beside the panel stage k_pm_shard,
k_pm_s, k_pm_panels of the same flushes) come from a kernel trace of this program (rocprofv3 --kernel-trace
--stats -- python tools/regression_bench.py); the program itself prints one JSON line with the shape, the flush
count and the event time of the whole assembly stage (DCFM_K_ASSEMBLE) per flush."""
import argparse
import json
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
    ap.add_argument("--thin", type=int, default=5)
    ap.add_argument("--asm-batch", type=int, default=32)
    ap.add_argument("--flushes", type=int, default=3)
    ap.add_argument("--q", type=int, default=32, help="responses (0: the flag alone, nothing set)")
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
    per_flush = args.thin * args.asm_batch
    smp = dcfm.Sampler(n, P, g, K, 0.5, 0, args.flushes * per_flush, args.thin, seed=1, asm_batch=args.asm_batch,
                       regression=True)
    ms = []
    try:
        smp.set_data_raw(Y, dcfm.shard_columns(keep, init.varind, P, 0, g))
        smp.init_state()
        if args.q:
            smp.set_regression((np.arange(args.q, dtype=np.int64) * p) // args.q)
        for f in range(args.flushes):
            smp.set_profiling_kernels(["k_assemble"])
            smp.run(1 + f * per_flush, per_flush)
            smp.synchronize()
            t, cnt = smp.kernel_stats()["k_assemble"]
            assert cnt >= 1, cnt
            ms.append(round(t / cnt, 3))
        assert smp.saved_samples() == args.flushes * args.asm_batch
        reg = smp.regression()
        if args.q:
            assert reg["count"] == args.flushes * args.asm_batch and np.all(np.isfinite(reg["coef"]))
            assert np.all(reg["r2"] > 0) and np.all(reg["r2"] < 1)
    finally:
        smp.close()
    print(json.dumps({"p": p, "g": g, "P": P, "K": K, "n": n, "thin": args.thin, "asm_batch": args.asm_batch,
                      "flushes": args.flushes, "q": args.q, "assemble_stage_ms_per_flush": ms,
                      "r2_mean": [round(float(v), 4) for v in reg["r2"][:4]]}))


if __name__ == "__main__":
    main()
