"""GPU parity at every BASELINE.json shape (configs c1-c4), not only at toy sizes.

The HIP path (through the C ABI) runs 2 iterations with injected draws (burn-in 1, one
saved sample, so the covariance assembly runs too) against the vectorised oracle
(oracle/vectorised.py, itself pinned to the faithful per-row loop in tests/test_oracle.py,
including at c1's shape).  Every state array after every iteration, and Sigmaout
(compared stripe by stripe through dcfm_get_sigma_cols, so the host never holds two
copies of p x p), must match to the north_star bar of 1e-10 normwise relative
(max |gpu - oracle| / max |oracle|).  Reference lines: dc:90-196.

  c1  p = 1,000   n = 100    g = 4   K = 5     (configs[0], the plumbing case)
  c2  p = 5,000   n = 500    g = 8   K = 20    (configs[1])
  c3  p = 19,968  n = 1,000  g = 64  K = 30    (configs[2], north star)
  c4  p = 10,000  n = 2,000  g = 8   K = 100   (configs[3], one chain)

Conditioning.  The reference chain's second iteration is not always well conditioned: with
quirks Q1 (Omega as a variance) and Q2 (the (R R')^-1 operator) the X / Z draws make
excursions (|X| ~ 1e3 at c2), E = eta'eta reaches cond ~1e7 and so does Q_j of the loading
rows (dc:141); any two restatements' Lambda then differ by cond x eps (the faithful loop and
the vectorised oracle by 1.3e-9 at c2).  Where that happens (c1, c2 iteration 2) the bars are
absolute and stage-wise (tests/helpers.stagewise_errors, the same check that pins the
vectorised oracle to the faithful loop at c2 / c3 in tests/test_oracle.py): the stages
before the loading solve (Z, X, eta) at 1e-10 against the oracle; the loading draw by its
per-row backward error against the oracle's systems Q_j, b_j, L_j, z_j (<= 1e-13); psi,
delta / tau, Plam at 1e-10 against the oracle update applied to the GPU's own Lambda; and
Sigmaout at 1e-10 against the oracle assembly of the GPU's own Lambda and omega.  No bar is
defined relative to another implementation.  Iteration 1 everywhere, and c3 / c4
throughout, keep the direct 1e-10 comparison.

ps and omega (dc:168-172), at every iteration of every case: per row, UNSCALED relative error
<= 1e-10 against the faithful loop's direct-residual update (dc:169 Ytil = Yd - eta Lambda')
applied to the GPU's own eta and Lambda; the oracle chain takes the residual too
(oracle.vectorised direct=True).  Two modes, c1-c4 each:
  exact    DCFM_FLAG_EXACT_RESIDUAL: every loading row's ps, omega from the direct residual on the
           device (k_resid64 for K <= 32, k_resid above: resid.hip);
  default  the throughput path: SS_j by the identity yy_j - 2 lam_j.C_j + lam_j E lam_j' inside the
           loading-row kernel, except where its cancellation could cost more than ~1e3 eps (the
           kappa guard, ss_identity_reject in resid.h): those waves take the direct residual for their
           8 rows (resid_rows8 in resid.h, same launch).  At c2's second
           iteration the identity alone is 1.3e-10 off (kappa_j ~ 1e6: its error grows like
           kappa_j eps, the residual's like sqrt(kappa_j) eps); the guard sends those rows to the
           residual; the wide path (c4, K = 100) has the same guard, its rejected rows' 32-row tiles
           redone by dc:169 in k_resid_flagged.
  guard_all DCFM_FLAG_GUARD_ALL: the guard rejects every row, so every row goes through the default
           path's own fallback (c2: resid_rows8 inside k_lambda; c4: every tile through
           k_resid_flagged) -- the code the default path runs only in transients, at the same bar.
           tests/test_gpu_resid_paths.py pins the same paths against each other at small shapes.
"""
import numpy as np
import pytest

from helpers import (STATE_CMP, make_case, ps_direct_err, rel_err, sigma_stripe_from_lower, stacked_draws,
                     stagewise_errors, state_dict)
from oracle import vectorised as V

pytestmark = pytest.mark.gpu

TOL = 1e-10
CONFIGS = {
    # name: (n, p, g, K, stage-wise bars at iteration 2)
    "c1": (100, 1000, 4, 5, True),
    "c2": (500, 5000, 8, 20, True),
    "c3": (1000, 19968, 64, 30, False),
    "c4": (2000, 10000, 8, 100, False),
}
EXACT = 0x10          # DCFM_FLAG_EXACT_RESIDUAL
GUARD_ALL = 0x40      # DCFM_FLAG_GUARD_ALL: the guard's residual fallback for every row (narrow and wide)
MODE_FLAGS = {"exact": EXACT, "default": 0, "guard_all": GUARD_ALL}
CASES = ([(name, mode) for mode in ("exact", "default") for name in CONFIGS] +
         [("c2", "guard_all"), ("c4", "guard_all")])


def _sigma_err(smp, SigL, p, w=2048):
    den = float(np.max(np.abs(np.diag(SigL))))        # max |Sigmaout| sits on the diagonal (SPD)
    worst = 0.0
    for c0 in range(0, p, w):
        c1 = min(p, c0 + w)
        S = smp.get_sigma_cols(c0, c1 - c0)
        if c0 == 0:
            assert np.array_equal(S[:c1, :], S[:c1, :].T), "Sigmaout not symmetric"
        worst = max(worst, float(np.max(np.abs(S - sigma_stripe_from_lower(SigL, c0, c1)))) / den)
    return worst


BW_TOL = 1e-13    # per-row backward error of the loading draw (helpers.loading_backward_error)


@pytest.mark.parametrize("name,mode", CASES)
def test_baseline_shape_parity(dcfm, name, mode):
    n, p, g, K, stagewise = CONFIGS[name]
    burnin, mcmc, thin = 1, 1, 1
    N = burnin + mcmc
    effsamp = mcmc / thin
    c = make_case(n, p, g, K, seed=29, k0=10, dense_truth=False)
    st, Yd = c["st"], c["Yd"]
    D = V.Data(Yd)
    smp = dcfm.Sampler(c["n"], c["P"], g, K, c["rho"], burnin, mcmc, thin, inject_draws=True,
                       flags=MODE_FLAGS[mode])
    try:
        smp.set_data(Yd)
        smp.set_state({f: v for f, v in state_dict(st).items() if f != "eta"})
        smp.set_draws(stacked_draws(c["src"], 1, N), 1, N)
        ref = st.copy()
        SigL = None
        for it in range(1, N + 1):
            start = ref.copy()
            smp.run(it, 1)
            SigL = V.run_chain(D, ref, c["rho"], c["hyper"], c["src"].iteration, it, 1,
                               burnin, mcmc, thin, SigLower=SigL, direct=True)
            got = smp.get_state()
            e = ps_direct_err(got, start, D.Yd, c["hyper"], c["src"].iteration(it))
            assert e < TOL, f"{name} {mode} iter {it}: ps / omega vs dc:169 residual, per row {e:.3e} (bar {TOL:.0e})"
            if it > 1 and stagewise:
                errs, bw, _, (sbw, cond) = stagewise_errors(start, got, D, c["rho"], c["hyper"], c["src"].iteration(it),
                                                            scaled=True)
                # printed beside the asserted normwise figure, not asserted: c1 / c2's conditioning has not been
                # measured against the reference (tests/test_loading_measure.py)
                print(f"CONFIG_STAGEWISE {name} {mode} iter {it}: lambda_bw {bw:.2e} lambda_sbw {sbw.max():.2e} "
                      f"cond(DQD) <= {cond.max():.2e}")
                for f, e in errs.items():
                    assert e < TOL, f"{name} iter {it}: stage {f} rel err {e:.3e} (bar {TOL:.0e})"
                assert bw < BW_TOL, f"{name} iter {it}: loading backward error {bw:.3e} (bar {BW_TOL:.0e})"
                # the assembly stage (dc:182-195) of the GPU's own Lambda and omega
                own = ref.copy()
                own.Lambda[...] = got["Lambda"]
                own.omega[...] = got["omega"]
                SigL = V.assemble_lower(np.zeros_like(SigL), own, c["rho"], effsamp)
                continue
            for f in STATE_CMP:
                e = rel_err(got[f], getattr(ref, f))
                assert e < TOL, f"{name} iter {it}: {f} rel err {e:.3e} (bar {TOL:.0e})"
        assert smp.saved_samples() == 1
        e = _sigma_err(smp, SigL, c["p"])
        assert e < TOL, f"{name}: Sigmaout rel err {e:.3e} (bar {TOL:.0e})"
    finally:
        smp.close()


@pytest.mark.timeout(900)
def test_c5_sweep_parity(dcfm, record_property):
    """configs[4] (c5: p = 100,096 = 391 x 256, n = 2,000, g = 256, K = 30) at its own
    shape: one injected-draw iteration of the sweep (dc:97-177) with thin > N, so Sigmaout (80 GB
    dense at this p; its assembly is pinned at this shape by test_gpu_scale.py) is skipped.  Every
    state array against the vectorised oracle at 1e-10 normwise, the stages of helpers.stagewise_errors
    (Z, X, eta; the loading draw's backward error; psi, delta / tau, Plam from the GPU's own Lambda;
    ps / omega per row against dc:169's direct residual), default (SS-identity) path."""
    n, p, g, K = 2000, 100096, 256, 30
    c = make_case(n, p, g, K, seed=29, k0=10, dense_truth=False)
    st, Yd = c["st"], c["Yd"]
    D = V.Data(Yd)
    smp = dcfm.Sampler(c["n"], c["P"], g, K, c["rho"], 0, 1, 10, inject_draws=True, asm_batch=1)
    try:
        smp.set_data(Yd)
        smp.set_state({f: v for f, v in state_dict(st).items() if f != "eta"})
        smp.set_draws(stacked_draws(c["src"], 1, 1), 1, 1)
        smp.run(1, 1)
        got = smp.get_state()
        assert smp.saved_samples() == 0
    finally:
        smp.close()
    start = st.copy()
    ref = st.copy()
    V.run_chain(D, ref, c["rho"], c["hyper"], c["src"].iteration, 1, 1, 0, 1, 10, SigLower=np.zeros((1, 1)),
                direct=True)
    errs = {f: rel_err(got[f], getattr(ref, f)) for f in STATE_CMP}
    stage, bw, _ = stagewise_errors(start, got, D, c["rho"], c["hyper"], c["src"].iteration(1))
    ps_row = ps_direct_err(got, start, D.Yd, c["hyper"], c["src"].iteration(1))
    record_property("c5_state_rel_err", errs)
    record_property("c5_stage_rel_err", {**stage, "lambda_bw": bw, "ps_direct_per_row": ps_row})
    print("C5_PARITY", {k: f"{v:.2e}" for k, v in {**errs, **{"stage_" + s: e for s, e in stage.items()},
                                                    "lambda_bw": bw, "ps_direct_per_row": ps_row}.items()})
    for f, e in errs.items():
        assert e < TOL, f"c5: {f} rel err {e:.3e} (bar {TOL:.0e})"
    for f, e in stage.items():
        assert e < TOL, f"c5: stage {f} rel err {e:.3e} (bar {TOL:.0e})"
    assert bw < BW_TOL, f"c5: loading backward error {bw:.3e}"
    assert ps_row < TOL, f"c5: ps / omega vs dc:169 residual, per row {ps_row:.3e}"
