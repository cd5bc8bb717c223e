"""Shared setup of the Sigmaout-operator tests (test_gpu_sigma_apply.py, test_gpu_sigma_eigs.py): a
short chain with saved samples per shape, its Sigmaout read back once as the host reference, and
the two-rank loopback harness."""
import threading

import pytest

from helpers import make_case, stacked_draws, state_dict

BURNIN, MCMC, THIN = 2, 6, 2
_made = {}


def run_sampler(dcfm, shape, **kw):
    n, p, g, K = shape
    c = make_case(n, p, g, K, seed=21, k0=4)
    smp = dcfm.Sampler(c["n"], c["P"], g, K, c["rho"], BURNIN, MCMC, THIN, seed=7, **kw)
    smp.set_data(c["Yd"])
    smp.set_state({k: v for k, v in state_dict(c["st"]).items() if k != "eta"})
    smp.run(1, BURNIN + MCMC)
    return smp


@pytest.fixture(scope="session")
def cases(dcfm):
    """shape -> (sampler, its Sigmaout read back): built once for both test files, never modified."""
    made = _made

    def get(shape):
        if shape not in made:
            smp = run_sampler(dcfm, shape)
            made[shape] = (smp, smp.get_sigma())
        return made[shape]

    yield get
    for smp, _ in made.values():
        smp.close()
    made.clear()


def loopback_pair(dcfm, work, n=60, p=400, g=4, K=5):
    """Two loopback ranks of one chain on one device, run to their saved samples; work(rank, sampler)
    runs on each rank's own thread (collective calls).  Returns the two results."""
    n_r = 2
    c = make_case(n, p, g, K, seed=23, k0=4)
    burnin, mcmc, thin = 1, 6, 2
    N = burnin + mcmc
    G = g // n_r
    draws = stacked_draws(c["src"], 1, N)
    smps = [dcfm.Sampler(c["n"], c["P"], g, K, c["rho"], burnin, mcmc, thin, inject_draws=True,
                         nranks=n_r, rank=r, device=0) for r in range(n_r)]
    out, errs = [None] * n_r, []
    try:
        dcfm.Sampler.comm_loopback(smps)
        for r, smp in enumerate(smps):
            smp.set_data(c["Yd"][:, :, r * G:(r + 1) * G])
            st = state_dict(c["st"], r * G, G)
            smp.set_state({f: st[f] for f in st if f != "eta"})
            smp.set_draws(draws, 1, N)

        def run(r):
            try:
                smps[r].run(1, N)
                out[r] = work(r, smps[r])
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
    return out
