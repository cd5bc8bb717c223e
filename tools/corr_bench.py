#!/usr/bin/env python3
"""Flushes of the correlation stage (DCFM_FLAG_CORR) beside its yardsticks, at the bench shape c3
(p = 19,968, g = 64, K = 30, thin 5, asm_batch 96: the steady-state 96-sample flush) by default, on a handle
set up the way bench.py sets one up (synthetic sparse-factor data, on-device ingest and initial state).
DCFM_FLAG_SIGMA_M2 and DCFM_FLAG_PARTIAL_CORR are on beside DCFM_FLAG_CORR, so one run holds k_assemble_m2,
k_assemble_pc_m2 and k_corr over the same tile list and k extents.  The per-kernel times come from a kernel
trace of this program (rocprofv3 --kernel-trace --stats -- python tools/corr_bench.py); the program itself prints
one JSON line with the shape, the flush count and the event time of the whole assembly stage (DCFM_K_ASSEMBLE)
per flush.  --no-corr / --no-yardsticks drop one side (the stage's own event time by difference)."""
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
    ap.add_argument("--asm-batch", type=int, default=96)
    ap.add_argument("--flushes", type=int, default=3)
    ap.add_argument("--no-corr", action="store_true")
    ap.add_argument("--no-yardsticks", action="store_true")
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
    yard = not args.no_yardsticks
    smp = dcfm.Sampler(n, P, g, K, 0.5, 0, args.flushes * per_flush, args.thin, seed=1, asm_batch=args.asm_batch,
                       sigma_m2=yard, partial_corr=yard, corr=not args.no_corr)
    ms = []
    try:
        smp.set_data_raw(Y, dcfm.shard_columns(keep, init.varind, P, 0, g))
        smp.init_state()
        for f in range(args.flushes):
            smp.set_profiling_kernels(["k_assemble"])
            smp.run(1 + f * per_flush, per_flush)
            smp.synchronize()
            t, cnt = smp.kernel_stats()["k_assemble"]
            assert cnt >= 1, cnt
            ms.append(round(t / cnt, 3))
        assert smp.saved_samples() == args.flushes * args.asm_batch
        block = smp.sigma_block()["bytes"]
        if not args.no_corr:
            h = smp.get_communality("mean")
            assert np.all(np.isfinite(h)) and np.all(h > 0) and np.all(h < 1)
    finally:
        smp.close()
    print(json.dumps({"p": p, "g": g, "P": P, "K": K, "n": n, "thin": args.thin, "asm_batch": args.asm_batch,
                      "flushes": args.flushes, "corr": not args.no_corr, "yardsticks": yard,
                      "sigma_block_bytes": block, "assemble_stage_ms_per_flush": ms}))


if __name__ == "__main__":
    main()
