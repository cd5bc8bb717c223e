"""Shared setup of the exact-replay tests (test_replay_plan.py on the CPU, test_gpu_replay.py on the GPU).

A generated-draw chain is a function of its seed alone: every variate is addressed by its counter (site,
shard, row, index, iteration; csrc/philox.h) and no kernel sums with atomics.  So one chain must come out
bit for bit however a run of N iterations is cut into dcfm_run calls, however the host overlaps its
streams, and however the draws and the saved samples are batched.  This module holds the run shape, the
call plans, the host model of what the schedule code in csrc/dcfm.hip does with a plan (which iterations
are saved, after which a flush is queued, how DrawBatches groups the generated draws), the layouts, and
the runners that drive a plan on one handle or on loopback ranks.

Run shape: N = 27, burnin 3, thin 2, assembly batches of 2.  Saved iterations 4, 6, .., 26 (12 samples);
one call flushes full batches after 6, 10, 14, 18, 22, 26 and forms the draw batches [1-8], [9-16],
[17-24], [25-27], so both draw slots and both Lb buffers are written more than once.
"""
import functools
import threading

import numpy as np

from helpers import make_case, state_dict

N, BURNIN, THIN, ASM_BATCH = 27, 3, 2, 2
MCMC = N - BURNIN
CHAIN_SEED, CASE_SEED = 77, 5
DRAW_BATCH = 8                                   # DrawBatches: iterations per k_draws batch (h->DB)
UNFUSED, ONE_STREAM = 0x2, 0x4                   # include/dcfm.h: DCFM_FLAG_UNFUSED, DCFM_FLAG_ONE_STREAM

# call plans: lists of (first_iter, n_iter)
ONE = [(1, 27)]
# every call ends where the unsplit run has just flushed a full batch (same flushes, same summation
# order of Sigmaout); the cuts at 7, 15 and 23 fall inside the unsplit run's draw batches [1-8], [9-16],
# [17-24], and the cut at 7 leaves the first call a batch of 6, short of DrawBatches' 8
ALIGNED = [(1, 6), (7, 8), (15, 8), (23, 5)]
# cuts inside assembly batches (4 | 6, 26 | end) and inside draw batches, a one-iteration and an empty call
RAGGED = [(1, 3), (4, 1), (5, 9), (14, 0), (14, 11), (25, 3)]
STEPPED = [(t, 1) for t in range(1, N + 1)]
PLANS = {"ONE": ONE, "ALIGNED": ALIGNED, "RAGGED": RAGGED, "STEPPED": STEPPED}


def is_saved(it, burnin=BURNIN, thin=THIN):
    return it % thin == 0 and it > burnin                          # dc:180


def saved_iterations(plan, burnin=BURNIN, thin=THIN):
    """The iterations whose sample is saved, in the order the plan runs them."""
    return [it for first, n in plan for it in range(first, first + n) if is_saved(it, burnin, thin)]


def flush_points(plan, burnin=BURNIN, thin=THIN, asm_batch=ASM_BATCH):
    """The iterations after which an assembly batch is handed over (save_sample: a full batch; dcfm_run's
    end: whatever the open batch holds, reported at the call's last iteration)."""
    out, batch = [], 0
    for first, n in plan:
        for it in range(first, first + n):
            if is_saved(it, burnin, thin):
                batch += 1
                if batch == asm_batch:
                    out.append(it)
                    batch = 0
        if batch:
            out.append(first + n - 1)
            batch = 0
    return out


def draw_batches(plan, DB=DRAW_BATCH):
    """(b0, nb) of every k_draws batch as DrawBatches forms them: aligned to each call's first iteration,
    DB iterations a batch, the last one of a call shorter."""
    out = []
    for first, n in plan:
        for b0 in range(first, first + n, DB):
            out.append((b0, min(DB, first + n - b0)))
    return out


# layouts: (n, p, g, K) of helpers.make_case and the create flags.  At these shapes the reference itself
# is well conditioned over all 27 iterations (test_replay_plan.test_reference_is_well_conditioned);
# (100, 180, 2, 70), (200, 180, 2, 70) and (250, 130, 2, 65) are not (max|X| 1e3-2e5 at iteration 2).
LAYOUTS = {
    "wide64": ((80, 96, 4, 40), 0),              # K > 32, 64-wide state rows
    "wide128": ((300, 160, 2, 66), 0),           # 128-wide: three 128-row tiles, 9 k-groups (2 over a 16-block)
    "unfused": ((37, 60, 3, 7), UNFUSED),        # K <= 32 through the side-stream schedule
    "fused": ((64, 160, 4, 30), 0),              # the fused K <= 32 chain
    "unfused30": ((64, 160, 4, 30), UNFUSED),    # the rank tests' side-schedule twin of "fused"
}
EXPECTED_NP = {"wide64": (80, 24), "wide128": (300, 80), "unfused": (37, 20), "fused": (64, 40),
               "unfused30": (64, 40)}


@functools.lru_cache(maxsize=None)
def case(layout):
    """make_case of the layout (cached; its arrays are shared, so read-only)."""
    (n, p, g, K), _ = LAYOUTS[layout]
    c = make_case(n, p, g, K, seed=CASE_SEED)
    c["Yd"].setflags(write=False)
    for v in c["st"].as_dict().values():
        v.setflags(write=False)
    return c


def layout_flags(layout):
    return LAYOUTS[layout][1]


def init_state(c, s0=0, gl=None):
    return {f: v for f, v in state_dict(c["st"], s0, gl).items() if f != "eta"}


def probe_vectors(p, nv, seed):
    return np.random.default_rng(seed).standard_normal((p, nv))


def _sampler(dcfm, layout, c, *, flags, asm_batch, burnin, features, nranks=1, rank=0):
    g, K = c["g"], c["K"]
    smp = dcfm.Sampler(c["n"], c["P"], g, K, c["rho"], burnin, N - burnin if burnin < N else 0, THIN,
                       seed=CHAIN_SEED, asm_batch=asm_batch, flags=layout_flags(layout) | flags, nranks=nranks,
                       rank=rank, sigma_m2=features, precision_mean=features)
    return smp


def _features_on(smp, p):
    smp.set_trace(N)
    smp.set_probes(probe_vectors(p, 3, 11))
    smp.set_precision_probes(probe_vectors(p, 2, 12))
    smp.set_loglik()


def _read(smp, features, out=None):
    out = {} if out is None else out
    out["state"] = smp.get_state()
    out["sigma"] = smp.get_sigma()
    out["saved"] = smp.saved_samples()
    if features:
        out["trace"] = smp.get_trace()
        out["probes"] = smp.probe_draws()
        out["prec_q"], out["prec_logdet"] = smp.precision_draws()
        _, out["ll_maha"], out["ll_logdet"] = smp.loglik_draws(parts=True)
        out["m2"] = smp.get_sigma_moment("m2")
        out["prec_mean"] = smp.get_precision_mean()
    return out


def run_plan(dcfm, layout, plan, *, flags=0, asm_batch=ASM_BATCH, burnin=BURNIN, features=False, sync=False,
             states=False, profiling=False):
    """The plan on a fresh handle, generated draws.  Returns {"state" (every STATE_FIELDS member),
    "sigma", "saved"} and, with `features`, the trace rows, the probe / precision / log-likelihood draws,
    the second moment and the precision mean.  `sync`: synchronize() after every call; `states`: also
    "states", the state before the first call and after every call; `profiling`: "stats", kernel_stats()
    of the whole plan timed at stride 1."""
    c = case(layout)
    smp = _sampler(dcfm, layout, c, flags=flags, asm_batch=asm_batch, burnin=burnin, features=features)
    out = {}
    try:
        smp.set_data(c["Yd"])
        smp.set_state(init_state(c))
        if features:
            _features_on(smp, c["P"] * c["g"])
        if profiling:
            smp.set_profiling(True)
        if states:
            out["states"] = [smp.get_state()]
        for first, n in plan:
            smp.run(first, n)
            if sync:
                smp.synchronize()
            if states:
                out["states"].append(smp.get_state())
        _read(smp, features, out)
        if profiling:
            out["stats"] = {k: v[1] for k, v in smp.kernel_stats().items()}
    finally:
        smp.close()
    return out


def run_plan_ranks(dcfm, layout, plan, nranks, *, flags=0, asm_batch=ASM_BATCH, timeout=100):
    """The plan on `nranks` loopback ranks of one chain on one device (tests/test_gpu_loopback._run_ranks:
    one host thread per rank).  Returns one run_plan-style dict per rank; "sigma" is None off rank 0."""
    c = case(layout)
    g = c["g"]
    G = g // nranks
    smps = [_sampler(dcfm, layout, c, flags=flags, asm_batch=asm_batch, burnin=BURNIN, features=False,
                     nranks=nranks, rank=r) for r in range(nranks)]
    try:
        dcfm.Sampler.comm_loopback(smps)
        for r, smp in enumerate(smps):
            smp.set_data(c["Yd"][:, :, r * G:(r + 1) * G])
            smp.set_state(init_state(c, r * G, G))
        out, errs = [None] * nranks, []

        def work(r):
            try:
                for first, n in plan:
                    smps[r].run(first, n)
                out[r] = _read(smps[r], False)               # get_sigma is collective: rank 0 receives
            except Exception as e:                           # surfaced below
                errs.append(e)

        ths = [threading.Thread(target=work, args=(r,)) for r in range(nranks)]
        for t in ths:
            t.start()
        for t in ths:
            t.join(timeout=timeout)
        assert not any(t.is_alive() for t in ths), "a rank did not finish"
        assert not errs, errs
        return out
    finally:
        for smp in smps:
            smp.close()
