#!/usr/bin/env python3
"""Timing of the on-device solve (dcfm_sigma_solve) at the bench shape c3 (p = 19,968, g = 64, K = 30),
on a handle set up the way bench.py sets one up (synthetic sparse-factor data, on-device ingest and
initial state, a few saved samples).  Prints one JSON line.

  device     Sampler.sigma_solve(B, tol) for nv = 1, 32: wall time of a call (upload of B, the whole
             iteration, download of X) and its dev_ms, median and min..max of --repeats calls after
             --warmup; the columns' iteration counts and worst relres; device time per iteration
             (dev_ms over the passes of the call: max iters + 1 for the residual pass).
  host       the yardstick, what a caller could do before: the same recurrence driven from the host
             with Sampler.sigma_apply for W = Sigma P and NumPy for the vector algebra (every pass copies
             p x nv up and p x nv down), same B, tol and stop test, timed the same way.
  apply      dev_ms and wall time of one Sampler.sigma_apply pass at the same nv, in the same session:
             what a solve iteration is measured against.
  host_share 1 - (passes x apply dev_ms) / wall, for both paths.
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


def host_cg(smp, B, tol, max_iter):
    """The recurrence of csrc/sigma_solve.hip with the pass on the device and everything else in NumPy."""
    X, R, P = np.zeros_like(B), B.copy(), B.copy()
    bb = np.einsum("ij,ij->j", B, B)
    rr = bb.copy()
    done = ~(bb > 0)
    iters = np.zeros(B.shape[1], dtype=np.int64)
    passes = 0
    for _ in range(max_iter):
        W = smp.sigma_apply(P)
        passes += 1
        pw = np.einsum("ij,ij->j", P, W)
        live = ~done & (pw > 0) & np.isfinite(pw)
        alpha = np.where(live, rr / np.where(live, pw, 1.0), 0.0)
        X += P * alpha
        R -= W * alpha
        rn = np.where(live, np.einsum("ij,ij->j", R, R), rr)
        done = ~live | (np.sqrt(rn) <= tol * np.sqrt(bb))
        beta = np.where(done, 0.0, rn / np.where(rr > 0, rr, 1.0))
        P = np.asfortranarray(np.where(done, P, R + P * beta))
        iters += live
        rr = rn
        if done.all():
            break
    relres = np.linalg.norm(B - smp.sigma_apply(X), axis=0) / np.sqrt(bb)
    return X, iters, relres, passes + 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--g", type=int, default=64)
    ap.add_argument("--P", type=int, default=312)
    ap.add_argument("--n", type=int, default=1000)
    ap.add_argument("--K", type=int, default=30)
    ap.add_argument("--iters", type=int, default=12, help="Gibbs iterations (thin 2: half of them saved)")
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--tol", type=float, default=1e-8)
    ap.add_argument("--max-iter", type=int, default=1000)
    ap.add_argument("--nv", type=int, nargs="+", default=[1, 32])
    ap.add_argument("--no-host", action="store_true", help="skip the host-driven yardstick")
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
    out = {"p": p, "g": g, "K": K, "n": n, "tol": args.tol, "max_iter": args.max_iter, "saved": None, "nv": {}}
    try:
        smp.set_data_raw(Y, dcfm.shard_columns(keep, init.varind, P, 0, g))
        smp.init_state()
        smp.run(1, args.iters)
        smp.synchronize()
        out["saved"] = smp.saved_samples()
        rng = np.random.default_rng(0)
        for nv in args.nv:
            B = np.asfortranarray(rng.standard_normal((p, nv)))
            res = {}
            a_dev, a_wall = [], []
            for i in range(args.warmup + args.repeats):
                t0 = time.perf_counter()
                _, ms = smp.sigma_apply(B, return_ms=True)
                t1 = time.perf_counter()
                if i >= args.warmup:
                    a_dev.append(ms)
                    a_wall.append((t1 - t0) * 1e3)
            res["apply"] = {"dev_ms": med(a_dev), "wall_ms": med(a_wall)}
            pass_ms = res["apply"]["dev_ms"]["median"]
            wall, dev = [], []
            for i in range(args.warmup + args.repeats):
                t0 = time.perf_counter()
                X, info = smp.sigma_solve(B, tol=args.tol, max_iter=args.max_iter, return_info=True)
                t1 = time.perf_counter()
                if i >= args.warmup:
                    wall.append((t1 - t0) * 1e3)
                    dev.append(info["ms"])
            it = np.atleast_1d(info["iters"])
            passes = int(it.max()) + 1
            w, d = med(wall), med(dev)
            res["device"] = {"wall_ms": w, "dev_ms": d, "iters_min": int(it.min()), "iters_max": int(it.max()),
                             "relres_max": float(np.max(info["relres"])), "passes": passes,
                             "dev_ms_per_pass": round(d["median"] / passes, 4),
                             "over_apply_pass": round(d["median"] / passes / pass_ms, 4),
                             "host_share": round(1.0 - passes * pass_ms / w["median"], 4)}
            if not args.no_host:
                hwall = []
                for i in range(args.warmup + args.repeats):
                    t0 = time.perf_counter()
                    Xh, hit, hrel, hpasses = host_cg(smp, B, args.tol, args.max_iter)
                    t1 = time.perf_counter()
                    if i >= args.warmup:
                        hwall.append((t1 - t0) * 1e3)
                hw = med(hwall)
                res["host"] = {"wall_ms": hw, "iters_min": int(hit.min()), "iters_max": int(hit.max()),
                               "relres_max": float(hrel.max()), "passes": hpasses,
                               "host_share": round(1.0 - hpasses * pass_ms / hw["median"], 4),
                               "max_rel_diff_x": float(np.max(np.linalg.norm(Xh - X, axis=0) /
                                                              np.linalg.norm(X, axis=0)))}
                res["device_over_host_wall"] = round(w["median"] / hw["median"], 4)
            out["nv"][str(nv)] = res
    finally:
        smp.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
