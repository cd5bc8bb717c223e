"""Shared setup of the probe-draw tests (test_gpu_probes.py): probe blocks, a short injected chain with
probes set before it runs (one iteration per run call, the state read back after every saved one), the
host evaluation of V' Sigma(s) V with its rounding bound, and the two-rank loopback harness.
sigma_cases.loopback_pair runs its chain before it hands the sampler over; probes must be set first."""
import threading
from types import SimpleNamespace

import numpy as np

from helpers import make_case, stacked_draws, state_dict
from oracle import dc_oracle as F

BURNIN, MCMC, THIN = 1, 6, 2
N = BURNIN + MCMC
SAVED = [it for it in range(1, N + 1) if it % THIN == 0 and it > BURNIN]
EFFSAMP = MCMC / THIN
EPS = np.finfo(np.float64).eps


def probe_block(p, nv, seed=5):
    """p x nv seeded normals; from three columns on, column 1 is all zero and column 2 a unit vector."""
    V = np.random.default_rng(seed).standard_normal((p, nv))
    if nv >= 3:
        V[:, 1] = 0.0
        V[:, 2] = 0.0
        V[(7 * p) // 11, 2] = 1.0
    return V


def sample_sigma(Lambda, omega, rho):
    """Sigma(s) of dc:182-192 from Lambda (P x K x g) and omega (P x g), by the oracle."""
    return F.assemble_sample(SimpleNamespace(Lambda=np.asarray(Lambda), omega=np.asarray(omega)), rho)


def host_draw(V, Lambda, omega, rho):
    """(V' Sigma(s) V, its rounding bound).  Both this evaluation and the device's are sums of products:
    per entry a dot product over the P rows of a shard, the K factors (W enters twice) and the g shards,
    so each is within gamma |V|' (|Lambda| C |Lambda|' + Omega) |V| of the exact value and the two within
    4 (P + g + K + 4) eps T of each other."""
    P, K, g = Lambda.shape
    V = V.reshape(V.shape[0], -1)
    Q = V.T @ sample_sigma(Lambda, omega, rho) @ V
    T = np.abs(V).T @ sample_sigma(np.abs(Lambda), omega, rho) @ np.abs(V)
    return Q, 4.0 * (P + g + K + 4) * EPS * T


def start(dcfm, c, g, K, **kw):
    """A sampler on case c with its data, state and injected draws set, nothing run."""
    smp = dcfm.Sampler(c["n"], c["P"], g, K, c["rho"], BURNIN, MCMC, THIN, inject_draws=True, **kw)
    smp.set_data(c["Yd"])
    smp.set_state({f: v for f, v in state_dict(c["st"]).items() if f != "eta"})
    smp.set_draws(stacked_draws(c["src"], 1, N), 1, N)
    return smp


def run_probed(dcfm, shape, V, capacity=None, states=True, keep=False, case_seed=21, **kw):
    """The injected chain of `shape` = (n, p, g, K) with probes V, one iteration per run call (`states`:
    the state is read back after every saved one; else the chain runs in one call).  Returns
    {"draws", "states" (Lambda, omega after every saved iteration), "rho", "smp" (open, with keep)}."""
    n, p, g, K = shape
    c = make_case(n, p, g, K, seed=case_seed, k0=4)
    smp = start(dcfm, c, g, K, **kw)
    try:
        smp.set_probes(V, capacity)
        sts = []
        if not states:
            smp.run(1, N)
        for it in range(1, N + 1 if states else 0):
            smp.run(it, 1)
            if it in SAVED:
                sts.append(smp.get_state(("Lambda", "omega")))
        out = {"draws": smp.probe_draws(), "states": sts, "rho": c["rho"], "smp": smp if keep else None}
    finally:
        if not keep:
            smp.close()
    return out


def loopback_probed(dcfm, V, n=60, p=400, g=4, K=5):
    """Two loopback ranks of one injected chain on one device with probes V set before the run; each
    rank's probe_draws() (collective) from its own thread.  Returns (the two results, the case)."""
    n_r = 2
    c = make_case(n, p, g, K, seed=23, k0=4)
    G = g // n_r
    draws = stacked_draws(c["src"], 1, N)
    smps = [dcfm.Sampler(c["n"], c["P"], g, K, c["rho"], BURNIN, MCMC, THIN, inject_draws=True,
                         nranks=n_r, rank=r, device=0) for r in range(n_r)]
    out, errs = [None] * n_r, []
    try:
        dcfm.Sampler.comm_loopback(smps)
        for r, smp in enumerate(smps):
            smp.set_data(c["Yd"][:, :, r * G:(r + 1) * G])
            st = state_dict(c["st"], r * G, G)
            smp.set_state({f: st[f] for f in st if f != "eta"})
            smp.set_draws(draws, 1, N)
            smp.set_probes(V)

        def run(r):
            try:
                smps[r].run(1, N)
                out[r] = smps[r].probe_draws()
            except Exception as e:                                        # surfaced below
                errs.append(e)

        ths = [threading.Thread(target=run, args=(r,)) for r in range(n_r)]
        for t in ths:
            t.start()
        for t in ths:
            t.join(timeout=100)
        assert not any(t.is_alive() for t in ths), "a rank did not finish"
        assert not errs, errs
    finally:
        for smp in smps:
            smp.close()
    return out, c
