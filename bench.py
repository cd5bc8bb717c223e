#!/usr/bin/env python3
"""Benchmark: Gibbs iterations/sec of the divide-and-conquer factor sampler at c3.

Workload (BASELINE.json configs[2], the metric's configuration):
  p = 19,968 (P = 312 x g = 64 shards), n = 1,000, K = 30 factors per shard
  (k = 1,920), rho = 0.5, thin = 5.  burnin = 0 so covariance assembly (one
  saved sample every 5 iterations, flushed in batches of 16) is inside the timed
  region.  Synthetic sparse-factor data (seeded; no dataset ships with the
  reference).  One "step" = one Gibbs iteration (divideconquer.m:90-197) of the
  whole chain; with N GPUs the 64 shards are split N ways (strong scaling, RCCL
  all-gathers over xGMI for the cross-shard exchanges).

A plain run sets up, warms up, times the K steps and prints the result line (metric, value,
unit, ms_per_step, ...).  --full adds everything else the benchmark measures, each in a run of
its own outside the timed region: the per-kernel HIP-event pass and the roofline figures, the
ingest timings, the chain trace diagnostics, the covariance error against the synthetic truth
(this chain and a separate converged one) and the CPU baselines.  --dump-outputs DIR writes
what the timed path computed in its last step (dump_outputs).

Usage: python bench.py [--gpus N] [--steps K] [--warmup W] [--full] [--dump-outputs DIR]
       (N > 1: python -m torch.distributed.run --nproc-per-node N bench.py --gpus N ...)
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT))

METRIC = "Gibbs iters/sec (node) at p=20k,n=1k,g=64; cov-assembly MFMA util %"
FP64_MFMA_PEAK_TFLOPS = 78.6      # MI355X dense fp64 matrix (spec; = fp64 vector)
HBM_PEAK_GBS = 8000.0             # MI355X HBM3E spec


def synth_data(n, p, k0=10, sparsity=0.7, seed=20161209, factors=False):
    """Sparse-factor synthetic data: Y = F L0' + E (with ``factors``: also L0, sig2)."""
    r = np.random.Generator(np.random.PCG64(seed))
    L0 = r.standard_normal((p, k0))
    L0[r.random((p, k0)) < sparsity] = 0.0
    sig2 = r.uniform(0.2, 1.0, size=p)
    F = r.standard_normal((n, k0))
    Y = F @ L0.T + r.standard_normal((n, p)) * np.sqrt(sig2)[None, :]
    return (Y, L0, sig2) if factors else Y


def algorithmic_work(kname, d, n_launch_samples, fused_z=False):
    """(flops, bytes, bound) per launch — the minimum the reference maths needs.  fused_z: the
    K <= 32 fused chain's W pass also draws Z (k_wcol: W stays in registers; read X, write Z
    and the X message instead of writing W)."""
    n, P, K, G, p, nr = d["n"], d["P"], d["K"], d["G"], d["p"], d["nranks"]
    if kname == "k_wpass" and fused_z:
        return (2.0 * G * n * P * K + G * n * (4.0 * K * K + 2.0 * K * K),
                8.0 * (G * n * P + G * P * (K + 1) + n * K + 2 * G * n * K), "hbm")
    if kname == "k_wpass":     # W_m = Y_m (w o L_m): one fp64 read of Y, L, w; write W
        return 2.0 * G * n * P * K, 8.0 * (G * n * P + G * P * (K + 1) + G * n * K), "hbm"
    if kname == "k_cpass":     # [C|E] = [Y|eta]' eta: read Y, X, Z; write C, E
        return 2.0 * G * n * (P + K) * K, 8.0 * (G * n * P + n * K + G * n * K + G * P * K), "hbm"
    if kname == "k_assemble":  # lower triangle of sum_s coef.(L_s L_s') over the batch
        return float(p) * (p + 1) * n_launch_samples * K / nr, 16.0 * p * (p + 1) / 2 / nr, "mfma"
    if kname == "k_lambda":   # per row: read C, psi, NL, Gpsi (K each), ps, yy, Gps; write Lam, psi, cpart, ps, omega
        return G * P * (K ** 3 / 3.0 + 6.0 * K * K), 8.0 * G * P * (7 * K + 5), "mfma"
    if kname == "k_resid":    # dc:169 Ytil = Y - eta L': read Y, X, Z, L, Gps; write ps, omega
        return 2.0 * G * n * P * K, 8.0 * (G * n * P + n * K + G * n * K + G * P * K + 3 * G * P), "hbm"
    if kname == "k_zdraw":
        return G * n * (4.0 * K * K + 2.0 * K * K), 8.0 * G * n * 4 * K, "hbm"
    return 0.0, 0.0, "hbm"


def binding_roof(flops, nbytes):
    """The roof a kernel's algorithmic work hits first: "hbm" when moving its bytes at the
    HBM peak takes longer than its flops at the fp64 peak, else "mfma" (k_lambda is HBM-bound
    at K = 30 — 4.3 us of bytes vs 3.7 us of flops — and MFMA-bound at K = 100)."""
    if flops <= 0.0:
        return "hbm"
    return "hbm" if nbytes / (HBM_PEAK_GBS * 1e9) >= flops / (FP64_MFMA_PEAK_TFLOPS * 1e12) else "mfma"


def build_id():
    """Identity of the product build: sha256 over the sources libdcfm.so is compiled from
    (csrc/*.hip, csrc/*.h, the Makefile, include/dcfm.h).  PMC summaries carry it, so
    roofline.traffic is only ever taken from a profile of this exact build."""
    import hashlib
    h = hashlib.sha256()
    csrc = ROOT / "a-divide-and-conquer-strategy-for-high-dimensional-bayesian-factor-models_amd" / "csrc"
    files = sorted(list(csrc.glob("*.hip")) + list(csrc.glob("*.h")) + [csrc / "Makefile", ROOT / "include" / "dcfm.h"])
    for p in files:
        h.update(p.name.encode())
        h.update(p.read_bytes())
    return h.hexdigest()[:16]


def config_key(args, world):
    """The bench invocation a PMC summary must match (workload, flush sizes, step counts)."""
    return (f"g{args.g}_P{args.P}_n{args.n}_K{args.K}_thin{args.thin}_asm{args.asm_batch}_"
            f"steps{args.steps}_warmup{args.warmup}_gpus{world}{'_chains' if args.chains else ''}"
            f"{'_exact' if args.exact_residual else ''}"
            f"{'_flags%x' % args.layout_flags if args.layout_flags else ''}")


# HIP-event role name -> the kernel rocprofv3 records it under (the fused K <= 32 chain's W pass
# and Z draw run as roles of k_wcol)
PMC_KERNEL = {"k_wpass": "k_wcol"}


def pmc_traffic(kernel, build, key, launches):
    """HBM bytes per launch of `kernel` in the timed region, from a committed rocprofv3 PMC
    summary (profiles/*_pmc.json, tools/pmc_summary.py over separate FETCH_SIZE /
    WRITE_SIZE passes of this same bench command, FETCH_SIZE doubled per the gfx950 note
    of the MI355X microarchitecture guide) whose build id AND bench configuration equal
    this run's; the mean over the kernel's last `launches` dispatches (the timed region is
    the last part of the run).  (None, None) when no summary matches."""
    for f in sorted((ROOT / "profiles").glob("*_pmc.json")):
        try:
            doc = json.load(open(f))
        except (OSError, ValueError):
            continue
        if doc.get("build") != build or doc.get("config") != key:
            continue
        ks = doc.get("kernels", {})
        k = (ks.get(kernel) or ks.get(PMC_KERNEL.get(kernel, ""))
             or next((v for name, v in ks.items() if name.startswith(kernel + "_")), None))
        if not k:
            continue
        fe, wr = k.get("fetch_bytes_each"), k.get("write_bytes_each")
        if fe and wr:
            tot = [a + b for a, b in zip(fe, wr)]
            if kernel in PMC_KERNEL:   # a run's last k_wcol is its column-sum-only launch, not a W pass
                big = max(tot)
                while tot and tot[-1] < 0.1 * big:
                    tot.pop()
            if len(tot) >= launches:
                return sum(tot[-launches:]) / launches, str(f.relative_to(ROOT))
        if k.get("hbm_bytes_per_dispatch") is not None:
            return k["hbm_bytes_per_dispatch"], str(f.relative_to(ROOT))
    return None, None


def _threads():
    try:
        from threadpoolctl import threadpool_info
        return max((i.get("num_threads", 1) for i in threadpool_info()), default=1)
    except Exception:
        return os.cpu_count() or 1


def _cpu_case(n, p, g, K, rho):
    import oracle
    from oracle import dc_oracle as F
    Y = synth_data(n, p)
    hyper = F.Hyper()
    Yk, n, pk, P, K_, keep = F.preprocess(Y, g, K * g)
    src = oracle.DrawSource(1, n, pk, g, K, hyper)
    init = src.init()
    Yd = F.standardize(F.partition(Yk, g, init.varind))
    st = F.initialise(n, P, K, g, rho, hyper, init)
    return Yd, st, src, hyper


def cpu_baseline_run(n, p, g, K, rho, steps=5, thin=5):
    """Vectorised NumPy restatement (oracle, 'port') on a bounded c3 sample.  The timed
    region includes the draw generation (the GPU leg draws its own numbers too)."""
    from oracle import vectorised as V
    Yd, st, src, hyper = _cpu_case(n, p, g, K, rho)
    D = V.Data(Yd)
    t0 = time.perf_counter()
    V.run_chain(D, st, rho, hyper, src.iteration, 1, steps, 0, steps, thin, direct=True)
    dt = time.perf_counter() - t0
    return {"value": steps / dt, "unit": "iter/s", "cores": int(_threads()), "kind": "port",
            "sample": f"{steps} Gibbs iterations of c3 (incl. {steps // thin} covariance assembly at thin={thin} "
                      f"and the draw generation), vectorised NumPy/OpenBLAS restatement of divideconquer.m:90-196 "
                      f"with dc:169's residual product as written (not MATLAB), {dt:.1f} s"}


def cpu_faithful_run(n, p, g, K, rho):
    """The MATLAB-structure CPU proxy: the faithful restatement
    (oracle/dc_oracle.py, the reference's per-shard, per-row loops of dc:97-177 kept as
    loops) for ONE Gibbs iteration of c3, draws generated inside the timed region.  A
    restatement, not MATLAB (no MATLAB on the box)."""
    from oracle import dc_oracle as F
    Yd, st, src, hyper = _cpu_case(n, p, g, K, rho)
    t0 = time.perf_counter()
    F.gibbs_iteration(st, Yd, rho, hyper, src.iteration(1))
    dt = time.perf_counter() - t0
    return {"value": 1.0 / dt, "unit": "iter/s", "cores": int(_threads()), "kind": "port",
            "sample": f"1 Gibbs iteration of c3 (no assembly), faithful per-row-loop NumPy restatement of "
                      f"divideconquer.m:97-177 (restatement, not MATLAB), {dt:.1f} s"}


DUMP_STATE_BYTES = 56_000_000      # state arrays: whole below this total, else each capped at 1/8 of it
DUMP_SIGMA_BYTES = 6_000_000       # Sigmaout: whole columns within this, at most 32 of them
DUMP_SEED = 20161209


def dump_outputs(smp, out_dir, suffix=""):
    """What a caller of the timed path receives after its last step, as out_dir/<name><suffix>.npy
    (float64, under 64 MB in all): every field of get_state() as <field>.npy, and Sigma_cols.npy,
    columns of Sigmaout (p x c: stripes of 8 adjacent columns a fixed seed picks, ascending; 32
    columns while p allows, DUMP_SIGMA_BYTES at most).  If the state exceeds
    DUMP_STATE_BYTES, each field larger than an eighth of that is cut to a fixed seeded sample of
    its elements (column-major order, ascending).  Same arguments, same build: same files."""
    out_dir.mkdir(parents=True, exist_ok=True)
    r = np.random.Generator(np.random.PCG64(DUMP_SEED))
    state = smp.get_state()
    whole = sum(a.nbytes for a in state.values()) <= DUMP_STATE_BYTES
    cap = DUMP_STATE_BYTES // 8 // 8
    for f, a in state.items():
        if not whole and a.size > cap:
            a = a.reshape(-1, order="F")[np.sort(r.choice(a.size, size=cap, replace=False))]
        np.save(out_dir / f"{f}{suffix}.npy", np.ascontiguousarray(a, dtype=np.float64))
    p = smp.P * smp.g
    ncols = int(min(32, p, max(1, DUMP_SIGMA_BYTES // (8 * p))))
    width = min(8, ncols)                                       # stripes of `width` adjacent columns
    starts = np.sort(r.choice(p // width, size=ncols // width, replace=False)) * width
    parts = [smp.get_sigma_cols(int(c), width) for c in starts]     # collective when the shards are split
    if parts[0] is not None:
        np.save(out_dir / f"Sigma_cols{suffix}.npy", np.ascontiguousarray(np.hstack(parts), dtype=np.float64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=480)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--thin", type=int, default=5)
    ap.add_argument("--asm-batch", type=int, default=96)
    ap.add_argument("--g", type=int, default=64)
    ap.add_argument("--P", type=int, default=312)
    ap.add_argument("--n", "--nobs", dest="n", type=int, default=1000)   # --nobs under torchrun (--n is ambiguous there)
    ap.add_argument("--K", type=int, default=30)
    ap.add_argument("--full", action="store_true",
                    help="also run what the headline figure does not need, outside the timed region: per-kernel "
                         "HIP-event pass + roofline, ingest timings, trace diagnostics, covariance error (this "
                         "chain and a converged one), CPU baselines; the options below this one shape those legs")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the state and a seeded sample of Sigmaout columns as "
                         "DIR/<name>.npy (float64, under 64 MB in all)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-steps", type=int, default=10)
    ap.add_argument("--no-faithful", action="store_true", help="skip the faithful-loop CPU leg (~30 s)")
    ap.add_argument("--no-profile", action="store_true", help="skip per-kernel HIP events")
    ap.add_argument("--timed-samples", type=int, default=4,
                    help="time this many launches of the roofline kernel inside the timed region, evenly "
                         "spaced (0 = every launch): each event pair leaves ~5 us of idle on the stream, "
                         "and events on all 20 of the driver's launches cost ~3 %% of the wall clock (DESIGN §5)")
    ap.add_argument("--layout-flags", type=lambda v: int(v, 0), default=0,
                    help="extra dcfm_config.flags layout bits (DCFM_FLAG_ONE_STREAM 0x4, "
                         "DCFM_FLAG_FLAT_PRIORITY 0x8, DCFM_FLAG_UNFUSED 0x2) for layout comparisons")
    ap.add_argument("--exact-residual", action="store_true",
                    help="DCFM_FLAG_EXACT_RESIDUAL: ps / omega from dc:169's direct residual (k_resid, one "
                         "more Y pass) instead of the SS identity; the parity mode, timed for its cost")
    ap.add_argument("--chains", action="store_true",
                    help="one independent chain per rank (config c4: parallel chains, seed 1 + rank, no "
                         "collectives; weak scaling) instead of splitting the shards of one chain")
    ap.add_argument("--err-iters", type=int, default=20,
                    help="Lanczos steps of the on-device truth error after the timed region (0: off)")
    ap.add_argument("--converged-burnin", type=int, default=1000)
    ap.add_argument("--converged-mcmc", type=int, default=5000,
                    help="after the timed region (1 GPU): a separate chain of burnin + mcmc iterations at the "
                         "same config whose posterior-mean Sigmaout error and split-R-hat / ESS are reported "
                         "(north_star check 2 at the BASELINE shape; 0: off)")
    args = ap.parse_args()

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")

    import torch
    import torch.distributed as dist
    if world > 1:
        # rendezvous + timing only (the data path is RCCL inside libdcfm).  Gloo prints its
        # "connected to N peer ranks" banner on fd 1; route it to stderr so stdout carries
        # exactly the one JSON line.
        sys.stdout.flush()
        saved_fd = os.dup(1)
        os.dup2(2, 1)
        try:
            dist.init_process_group("gloo")
        finally:
            sys.stdout.flush()
            os.dup2(saved_fd, 1)
            os.close(saved_fd)

    import __graft_entry__ as ge
    dcfm = ge.load_package()

    g, P, n, K, rho, thin = args.g, args.P, args.n, args.K, 0.5, args.thin
    p = g * P
    full = args.full
    n_prof = args.steps if full and not args.no_profile else 0     # untimed per-kernel profiling pass (--full)
    N = args.warmup + n_prof + args.steps
    burnin, mcmc = 0, N
    Y, L0, sig2 = synth_data(n, p, factors=True)
    hyper = dcfm.Hyper()
    ndev = max(1, torch.cuda.device_count())     # counting devices does not initialise the GPU
    device = local_rank % ndev
    # driver half on the device: dc:31-38 column scan, then dc:48-59
    # gather + standardise by dcfm_set_data_raw below; Y crosses PCIe once per call
    if full:
        dcfm.count_nonzero_columns(Y[:, :64], device=device)      # first launch loads the code object
    nnz, ms_nnz = dcfm.count_nonzero_columns(Y, device=device, return_ms=True)
    keep = np.flatnonzero(nnz != 0)
    pk = keep.size
    if pk % g:   # the reference errors here too (dc:41: p must split into g equal shards)
        raise SystemExit(f"{pk} non-zero columns do not split into g = {g} equal shards")
    P = pk // g
    init = dcfm.driver._HostVarind(1, pk)     # dc:50 on the host; dc:68-87 on the device below
    chains = args.chains
    shard_ranks = 1 if chains else world        # ranks that split one chain's shards
    gl = g // shard_ranks
    s0 = 0 if chains else rank * gl

    smp = dcfm.Sampler(n, P, g, K, rho, burnin, mcmc, thin, seed=1 + (rank if chains else 0),
                       nranks=shard_ranks, rank=0 if chains else rank, device=device,
                       asm_batch=args.asm_batch, flags=(0x10 if args.exact_residual else 0) | args.layout_flags)
    if shard_ranks > 1:
        obj = [dcfm.Sampler.unique_id() if rank == 0 else None]
        dist.broadcast_object_list(obj, src=0)
        smp.comm_init(obj[0])
    cols = dcfm.shard_columns(keep, init.varind, P, s0, gl)
    if full:
        smp.set_data_raw(Y, cols)             # first launches load the code objects
    t_ing = time.perf_counter()
    _, ms_std = smp.set_data_raw(Y, cols)
    t_ing = time.perf_counter() - t_ing
    ingest = {"k_nnz_cols_us": round(ms_nnz * 1e3, 1),
              "k_nnz_cols_gbs": round(8.0 * n * p / (ms_nnz * 1e-3) / 1e9, 1) if ms_nnz > 0 else None,
              "k_colstats_k_stdize_us": round(ms_std * 1e3, 1),
              "k_colstats_k_stdize_gbs": round(16.0 * n * P * gl / (ms_std * 1e-3) / 1e9, 1) if ms_std > 0 else None,
              "set_data_raw_ms_incl_pcie": round(t_ing * 1e3, 1),
              "note": "one-time, before the timed region; GB/s = algorithmic bytes (8np read for the scan; "
                      "8nP read + 8nP write per rank for stats + standardise) / kernel time, second call"}
    t_init = time.perf_counter()
    smp.init_state()                          # dcfm_init_state: Philox, iteration-0 counters
    ingest["init_state_ms"] = round((time.perf_counter() - t_init) * 1e3, 2)
    if full:
        U_true, s_true = dcfm.truth_factors(L0, sig2, Y, keep, init.varind)
    del Y

    have_torch_gpu = torch.cuda.is_available()
    def sync():
        smp.synchronize()
        if have_torch_gpu:
            torch.cuda.synchronize(device)   # this rank's GPU (without it every rank opens a context on GPU 0)

    def barrier():
        if world > 1:
            dist.barrier()

    # chain trace over the untimed warmup + profiling iterations only (--full)
    n_trace = args.warmup + n_prof if full else 0
    if n_trace >= 4:
        smp.set_trace(n_trace)
    smp.run(1, args.warmup)
    sync()
    # (1) untimed pass with HIP events around every launch: the per-kernel table.
    #     Events cost host time per launch, so this pass is not the throughput run.
    stats, dominant = {}, None
    first_t = args.warmup + 1
    if n_prof:
        smp.set_profiling(True)
        smp.run(first_t, n_prof)
        sync()
        stats = smp.kernel_stats()
        smp.set_profiling(False)
        main_chain = [k for k in stats if k not in ("rccl", "k_draws", "k_prep", "k_xchol")]
        dominant = max(main_chain, key=lambda k: stats[k][0])
        first_t += n_prof
    trace = None
    if n_trace >= 4:
        trace = smp.get_trace()
        smp.set_trace(0)                    # the timed region records nothing
    # (2) the timed region: events only around the roofline kernel (live duration); on every
    #     --timed-samples N launches (default 4 of the region's, evenly spaced; 0: every launch).
    #     A plain run has no per-kernel table, hence no roofline kernel and no events at all.
    prof_stride = 1 if dominant == "k_assemble" or args.timed_samples <= 0 else max(1, args.steps // args.timed_samples)
    if dominant:
        smp.set_profiling_kernels([dominant], stride=prof_stride)
    barrier(); sync()
    t0 = time.perf_counter()
    smp.run(first_t, args.steps)
    sync(); barrier()
    dt = time.perf_counter() - t0
    live = smp.kernel_stats().get(dominant) if dominant else None
    saved_prof = sum(1 for t in range(args.warmup + 1, args.warmup + 1 + n_prof) if t % thin == 0)
    saved_in_region = sum(1 for t in range(first_t, first_t + args.steps) if t % thin == 0)
    if args.dump_outputs:
        dump_outputs(smp, Path(args.dump_outputs), f".rank{rank}" if world > 1 else "")
    # (3) after the timed region: the posterior-mean covariance error against the synthetic
    #     truth on the device (dcfm_sigma_error) — one norms-only pass (its HBM rate: the full
    #     p x p read from the stored triangle, 8 p^2 bytes) and a Lanczos operator norm
    sig_err = None
    if full and args.err_iters > 0:
        sync()
        te = time.perf_counter()
        e0 = smp.sigma_error(U_true, s_true, iters=0)
        t_pass = time.perf_counter() - te
        te = time.perf_counter()
        e1 = smp.sigma_error(U_true, s_true, iters=args.err_iters)
        t_lz = time.perf_counter() - te
        sig_err = {"fro_rel": round(e0["fro_rel"], 6), "op": round(e1["op"], 6),
                   "lanczos_iters": args.err_iters, "pass_ms": round(t_pass * 1e3, 3),
                   "pass_gbs": round(8.0 * p * p / t_pass / 1e9, 1),
                   "lanczos_ms": round(t_lz * 1e3, 2),
                   "note": "after the timed region; chain of warmup+steps iterations, not converged"}
    smp.close()

    # (4) north_star check (2) at this shape: a converged chain (BURNIN 1,000,
    #     MCMC 5,000, thin 5) from its own init, outside the timed region; its posterior-mean
    #     Sigmaout against the synthetic truth, with split-R-hat / ESS of the MCMC part's trace
    converged = None
    if full and world == 1 and args.converged_mcmc > 0 and args.err_iters > 0:
        cb, cm = args.converged_burnin, args.converged_mcmc
        smc = dcfm.Sampler(n, P, g, K, rho, cb, cm, thin, seed=7, device=device, asm_batch=args.asm_batch)
        try:
            Yc, _, _ = synth_data(n, p, factors=True)
            smc.set_data_raw(Yc, cols)
            del Yc
            smc.init_state()
            smc.run(1, cb)
            smc.set_trace(cm)
            smc.synchronize()
            tc = time.perf_counter()
            smc.run(cb + 1, cm)
            smc.synchronize()
            tc = time.perf_counter() - tc
            ec0 = smc.sigma_error(U_true, s_true, iters=0)
            ec1 = smc.sigma_error(U_true, s_true, iters=max(args.err_iters, 40))
            summ = dcfm.diagnostics.summarize(smc.get_trace()[None])
            converged = {"burnin": cb, "mcmc": cm, "thin": thin, "saved_samples": smc.saved_samples(),
                         "fro_rel": round(ec0["fro_rel"], 6), "op": round(ec1["op"], 6),
                         "op_rel": round(ec1["op"] / float(np.linalg.norm(U_true, 2) ** 2 + 0.0), 6),
                         "split_rhat": {k: round(v["rhat"], 4) for k, v in summ.items()},
                         "ess": {k: round(v["ess"], 1) for k, v in summ.items()},
                         "mcmc_seconds": round(tc, 3),
                         "note": "separate chain (seed 7) at the bench config, outside the timed region; "
                                 "split-R-hat / ESS over the MCMC iterations' device trace; op_rel uses "
                                 "||U U'||_2 as the truth's scale (the diagonal term adds < 1)"}
        finally:
            smc.close()

    diag = None
    if trace is not None and len(trace) >= 4:
        tr = torch.from_numpy(np.ascontiguousarray(trace))
        if world > 1 and chains:            # one chain per rank: gather them all
            parts = [torch.zeros_like(tr) for _ in range(world)]
            dist.all_gather(parts, tr)
            traces = np.stack([q.numpy() for q in parts])
        else:                               # ranks split one chain: its rows add up
            if world > 1:
                dist.all_reduce(tr)
            traces = tr.numpy()[None]
        summ = dcfm.diagnostics.summarize(traces)
        diag = {"chains": int(traces.shape[0]), "iterations": int(traces.shape[1]),
                "split_rhat": {k: round(v["rhat"], 4) for k, v in summ.items()},
                "ess": {k: round(v["ess"], 1) for k, v in summ.items()},
                "note": "device trace (dcfm_set_trace) of the untimed warmup + profiling iterations; "
                        "split-R-hat / ESS per BDA3 over chains x split halves"}

    if world > 1:
        tt = torch.tensor([dt], dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        dt = float(tt.item())

    value = args.steps / dt * (world if chains else 1)     # chains: iterations of all chains
    bid, ckey = build_id(), config_key(args, world)
    d = {"n": n, "P": P, "K": K, "G": gl, "p": p, "nranks": shard_ranks}
    kern = {}
    roof = None
    fused_z = K <= 32 and stats.get("k_wpass", (0, 0))[1] > 0 and stats.get("k_zdraw", (0, 0))[1] == 0
    def work_of(name, cnt, saved, iters):
        """Algorithmic (flops, bytes, bound) per launch: per-iteration work spread over the
        launches of one iteration (the Y-pass / row kernels run as two shard groups)."""
        if name == "k_assemble":
            fl, by, _ = algorithmic_work(name, d, saved / max(cnt, 1))
            return fl, by, binding_roof(fl, by)
        fl, by, _ = algorithmic_work(name, d, 0, fused_z)
        per_iter = max(cnt, 1) / max(iters, 1)
        return fl / per_iter, by / per_iter, binding_roof(fl, by)

    if stats:
        for name, (ms, cnt) in stats.items():
            if cnt == 0:
                continue
            avg_s = ms / cnt / 1e3
            fl, by, bound = work_of(name, cnt, saved_prof, n_prof)
            kern[name] = {"ms_total": round(ms, 4), "launches": int(cnt), "avg_us": round(avg_s * 1e6, 2),
                          "gflops_per_launch": round(fl / 1e9, 4), "mb_per_launch": round(by / 1e6, 3),
                          "tflops": round(fl / avg_s / 1e12, 3) if avg_s > 0 else None,
                          "gbs": round(by / avg_s / 1e9, 1) if avg_s > 0 else None, "bound": bound}
    if live and live[1]:
        ms, cnt = live
        avg_s = ms / cnt / 1e3
        # the region's launches of the kernel (cnt of them timed): per-iteration launches from the
        # untimed pass, where every launch was timed
        region_n = cnt if prof_stride == 1 or not stats.get(dominant) else \
            max(cnt, round(stats[dominant][1] / max(n_prof, 1) * args.steps))
        fl, by, bound = work_of(dominant, region_n, saved_in_region, args.steps)
        if bound == "mfma":
            ach, peak, unit = fl / avg_s / 1e12, FP64_MFMA_PEAK_TFLOPS, "TFLOP/s"
        else:
            ach, peak, unit = by / avg_s / 1e9, HBM_PEAK_GBS, "GB/s"
        traffic, tsrc = pmc_traffic(dominant, bid, ckey, int(region_n))
        roof = {"kernel": dominant, "bound": bound, "achieved": round(ach, 3), "peak": peak, "unit": unit,
                "frac": round(ach / peak, 4),
                "traffic": round(traffic) if traffic is not None else None,
                "traffic_unit": "bytes/launch", "traffic_source": tsrc, "build": bid, "config_key": ckey,
                "algorithmic_bytes": round(by), "avg_us": round(avg_s * 1e6, 2),
                "launches": int(cnt), "launches_in_region": int(region_n), "timed_every": prof_stride,
                "note": "achieved = algorithmic work per launch / mean HIP-event duration of this kernel, "
                        "events recorded around it alone inside the timed region, on one in timed_every "
                        "of its launches"}

    wtag = {(64, 312, 1000, 30): "c3", (8, 1250, 2000, 100): "c4", (256, 391, 2000, 30): "c5"}.get(
        (g, P, n, K), "custom")
    out = {
        "metric": METRIC, "value": round(value, 2), "unit": "iter/s", "n_gpus": world,
        "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(dt / args.steps * 1e3, 4),
        "higher_is_better": True, "scaling": "weak" if chains else "strong", "vs_baseline": None, "dtype": "f64",
        "data": "synthetic (sparse factor model, seed 20161209; initial state dc:68-87 drawn on the device)",
        "config": {"workload": f"{wtag}: p={p} (P={P} x g={g}), n={n}, K={K} (k={K * g}), rho={rho}, "
                               f"thin={thin}, burnin=0 (assembly in timed region), asm_batch={args.asm_batch}"
                               f"{', exact residual (k_resid)' if args.exact_residual else ''}",
                   "global_batch": n,
                   "parallelism": f"chains{world} (1 per GPU)" if chains else f"shards{g}/gpus{world}"},
        "full": full,
        "build": bid,
        "config_key": ckey,
    }
    if full:
        out["roofline"] = roof
    if "k_assemble" in kern:
        out["assembly_mfma_util"] = round(kern["k_assemble"]["tflops"] / FP64_MFMA_PEAK_TFLOPS, 4)
    if full:
        out["kernels"] = kern
    if sig_err:
        out["sigma_error"] = sig_err
    if converged:
        out["sigma_error_converged"] = converged
    if full:
        out["ingest"] = ingest
    if diag:
        out["diagnostics"] = diag
    if full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline_run(n, p, g, K, rho, steps=args.cpu_steps, thin=thin)
        if not args.no_faithful:
            out["cpu_baseline_faithful"] = cpu_faithful_run(n, p, g, K, rho)
    if rank == 0:
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
