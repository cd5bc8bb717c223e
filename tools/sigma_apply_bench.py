#!/usr/bin/env python3
"""Timing of the Sigmaout operator (dcfm_sigma_apply, dcfm_sigma_eigs) at the bench shape c3
(p = 19,968, g = 64, K = 30), on a handle set up the way bench.py sets one up (synthetic
sparse-factor data, on-device ingest and initial state, a few saved samples).  Prints one JSON line.

  apply      device time (dev_ms: events around the two kernels) and wall time (with the PCIe copies
             of V and Y) of one call for nv = 1, 8, 32: median and min..max of --repeats calls after
             --warmup; achieved HBM rate on the traffic model 4 p^2 bytes (the stored triangle once).
  yardstick  one pass of k_sigma_err (the one-vector mat-vec of dcfm_sigma_error, 8 p^2 bytes): the
             wall time of dcfm_sigma_error with 3 Lanczos steps minus that with 1, halved -- two
             more passes, each with its 160 KB copies, as the apply's wall time has.
  eigs       dcfm_sigma_eigs(r, tol, max_passes): passes, wall time, and the host share of it
             (wall minus the device passes at the nv = 32 wall time above).
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def med(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--g", type=int, default=64)
    ap.add_argument("--P", type=int, default=312)
    ap.add_argument("--n", type=int, default=1000)
    ap.add_argument("--K", type=int, default=30)
    ap.add_argument("--iters", type=int, default=12, help="Gibbs iterations (thin 2: half of them saved)")
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--eigs-r", type=int, default=10)
    ap.add_argument("--eigs-tol", type=float, default=1e-8)
    ap.add_argument("--eigs-max-passes", type=int, default=20)
    ap.add_argument("--no-eigs", action="store_true")
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
    smp = dcfm.Sampler(n, P, g, K, 0.5, 0, args.iters, 2, seed=1)
    out = {"p": p, "g": g, "K": K, "n": n, "saved": None}
    try:
        smp.set_data_raw(Y, dcfm.shard_columns(keep, init.varind, P, 0, g))
        smp.init_state()
        smp.run(1, args.iters)
        smp.synchronize()
        out["saved"] = smp.saved_samples()
        rng = np.random.default_rng(0)
        tri_bytes = 4.0 * p * p
        out["apply"] = {}
        for nv in (1, 8, 32):
            V = np.asfortranarray(rng.standard_normal((p, nv)))
            dev, wall = [], []
            for i in range(args.warmup + args.repeats):
                t0 = time.perf_counter()
                _, ms = smp.sigma_apply(V, return_ms=True)
                t1 = time.perf_counter()
                if i >= args.warmup:
                    dev.append(ms)
                    wall.append((t1 - t0) * 1e3)
            d = med(dev)
            out["apply"][str(nv)] = {"dev_ms": d, "wall_ms": med(wall),
                                     "tbs_on_4p2_bytes": round(tri_bytes / (d["median"] * 1e-3) / 1e12, 3)}
        U = np.asfortranarray(0.1 * rng.standard_normal((p, 4)))
        s = rng.uniform(0.5, 1.0, p)
        t1s, t3s = [], []
        for i in range(args.warmup + args.repeats):
            t0 = time.perf_counter()
            smp.sigma_error(U, s, iters=1)
            t1 = time.perf_counter()
            smp.sigma_error(U, s, iters=3)
            t2 = time.perf_counter()
            if i >= args.warmup:
                t1s.append((t1 - t0) * 1e3)
                t3s.append((t2 - t1) * 1e3)
        per = [(b - a) / 2 for a, b in zip(t1s, t3s)]
        m = med(per)
        out["k_sigma_err_pass"] = {"wall_ms": m, "sigma_error_iters1_ms": med(t1s), "sigma_error_iters3_ms": med(t3s),
                                   "tbs_on_8p2_bytes": round(2 * tri_bytes / (m["median"] * 1e-3) / 1e12, 3)}
        if not args.no_eigs:
            t0 = time.perf_counter()
            e = smp.sigma_eigs(args.eigs_r, tol=args.eigs_tol, max_passes=args.eigs_max_passes, vectors=False)
            wall = (time.perf_counter() - t0) * 1e3
            dev = (e["passes"] + 1) * out["apply"]["32"]["wall_ms"]["median"]
            out["eigs"] = {"r": args.eigs_r, "tol": args.eigs_tol, "max_passes": args.eigs_max_passes,
                           "passes": e["passes"], "converged": e["converged"], "wall_ms": round(wall, 1),
                           "device_passes_ms": round(dev, 1), "host_share": round(1.0 - dev / wall, 4),
                           "values": [float(x) for x in e["values"]],
                           "resid_over_lambda1": [float(x / e["values"][0]) for x in e["resid"]]}
    finally:
        smp.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
