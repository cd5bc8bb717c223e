"""Oracle parity at every factor count K that selects its own kernel instantiation (tests/k_paths.py: the
census, the case list and the shapes; tests/test_k_paths.py checks the census against the launcher text and
the reference at every case, on the CPU).

One test per K.  Injected draws, the default mode, one iteration per call.  After each of the 3 iterations the
oracle is restarted from the device's own previous state and the iteration is measured stage-wise
(helpers.stagewise_errors), against the project's bars:
  X, Z, eta, psi, delta, tau, Plam     1e-10 normwise
  loading draw                         per-row backward error <= 1e-13
  ps, omega per row                    against dc:169 on the device's own eta and Lambda, within
                                       max(1e-10, helpers.residual_rounding_bound)
After the run Sigmaout is exactly symmetric and within 1e-12 normwise of (1 / effsamp) sum assemble_sample over
the device's own states at the two saved iterations, and saved_samples() is 2.

K = 12, 23, 89 and 112 (one K of each class nothing reached before) also run DCFM_FLAG_GUARD_ALL and
DCFM_FLAG_EXACT_RESIDUAL under the same assertions, and the guard's fallback must agree with the exact launch
per row within twice the rounding bound (as tests/test_gpu_resid_paths.py).

Measured on the MI355X: DESIGN.md section 2, "Every K-selected instantiation", with the outcome of a 1e-9
perturbation of k_lambda<24> and of k_lambda_w<128, 6>: K = 21, 23, 24, 88 and 96 fail on it, K = 81 and 89 do not.
The limit it shows: the loading bar is a normwise backward error, relative to ||Q_j|| ||lambda_j||, and at wide K
||Q_j|| is Plam's trailing diagonal (tau_K ~ 2^K), so that bar does not see a small relative error in the data part
of a wide factor; there the ps / omega bar of the default mode (the SS identity takes lambda' E lambda from the
factor) is what notices.
"""
import functools

import numpy as np
import pytest

import k_paths as kp
from helpers import (as_oracle_state, residual_rounding_bound, scaled_rel_err, stacked_draws, stagewise_errors,
                     state_dict)
from oracle import dc_oracle as F

pytestmark = pytest.mark.gpu

TOL = 1e-10           # the project's stage-wise bar
BW_TOL = 1e-13        # loading backward error
SIGMA_TOL = 1e-12     # Sigmaout against the host sum of the device's own samples


@functools.lru_cache(maxsize=None)
def _run(dcfm, K, mode):
    """The chain of case K in `mode`, one iteration per call: the states (the start first), Sigmaout and the
    saved-sample count.  Made once, shared, read only."""
    c = kp.case(K)
    n, P, g, _ = kp.shape(K)
    start = state_dict(c["st"])
    smp = dcfm.Sampler(n, P, g, K, c["rho"], kp.BURNIN, kp.MCMC, kp.THIN, inject_draws=True, flags=kp.MODES[mode])
    try:
        smp.set_data(c["Yd"])
        smp.set_state({f: v for f, v in start.items() if f != "eta"})
        smp.set_draws(stacked_draws(c["src"], 1, kp.N_ITER), 1, kp.N_ITER)
        states = [{f: np.array(v) for f, v in start.items()}]
        for it in range(1, kp.N_ITER + 1):
            smp.run(it, 1)
            states.append(smp.get_state())
        out = dict(states=states, sigma=smp.get_sigma(), saved=smp.saved_samples())
    finally:
        smp.close()
    for st in out["states"]:
        for v in st.values():
            v.setflags(write=False)
    out["sigma"].setflags(write=False)
    return out


def _check(dcfm, K, mode):
    c = kp.case(K)
    r = _run(dcfm, K, mode)
    states = r["states"]
    assert len(states) == kp.N_ITER + 1
    worst = {}
    for it in range(1, kp.N_ITER + 1):
        got = states[it]
        errs, bw, ref = stagewise_errors(as_oracle_state(states[it - 1]), got, c["Yd"], c["rho"], c["hyper"],
                                         c["src"].iteration(it))
        bound = residual_rounding_bound(got, c["Yd"]).T            # P x g, the ps / omega layout
        for f in ("ps", "omega"):
            worst[f + "_raw"] = max(worst.get(f + "_raw", 0.0), errs[f])
            errs[f] = scaled_rel_err(got[f], getattr(ref, f), bound, TOL)
        worst["ps_bound_max"] = max(worst.get("ps_bound_max", 0.0), float(bound.max()))
        worst["lambda_bw"] = max(worst.get("lambda_bw", 0.0), bw)
        for f, e in errs.items():
            worst[f] = max(worst.get(f, 0.0), e)
        print(f"K_PATHS {kp.case_id(K)} {mode} iter {it}:", {f: f"{e:.2e}" for f, e in sorted(errs.items())},
              f"lambda_bw {bw:.2e}")
        for f, e in errs.items():
            assert e < TOL, f"K = {K} {mode} iteration {it}: stage {f} rel err {e:.3e} (bar {TOL:.0e})"
        assert bw <= BW_TOL, f"K = {K} {mode} iteration {it}: loading backward error {bw:.3e} (bar {BW_TOL:.0e})"
    # Sigmaout (dc:180-195) from the device's own saved states
    S = r["sigma"]
    assert r["saved"] == kp.MCMC // kp.THIN == 2
    assert np.all(np.isfinite(S)) and np.array_equal(S, S.T), "Sigmaout not exactly symmetric"
    saved = [it for it in range(1, kp.N_ITER + 1) if it % kp.THIN == 0 and it > kp.BURNIN]
    want = sum(F.assemble_sample(as_oracle_state(states[it]), c["rho"]) for it in saved) / (kp.MCMC / kp.THIN)
    worst["sigma"] = float(np.max(np.abs(S - want)) / np.max(np.abs(want)))
    print(f"K_PATHS_WORST {kp.case_id(K)} {mode} classes {kp.classes(K)} shape {kp.shape(K)}:",
          {f: f"{e:.2e}" for f, e in sorted(worst.items())})
    assert worst["sigma"] < SIGMA_TOL, f"K = {K} {mode}: Sigmaout vs the device's own samples {worst['sigma']:.3e}"
    return worst


@pytest.mark.parametrize("K", kp.CASES, ids=kp.case_id)
def test_stagewise_parity(dcfm, K, record_property):
    for f, e in _check(dcfm, K, "default").items():
        record_property(f"worst_{f}", e)


@pytest.mark.parametrize("mode", ["guard_all", "exact"])
@pytest.mark.parametrize("K", kp.EXTRA_MODE_CASES, ids=kp.case_id)
def test_stagewise_parity_residual_modes(dcfm, K, mode, record_property):
    for f, e in _check(dcfm, K, mode).items():
        record_property(f"worst_{f}", e)


@pytest.mark.parametrize("K", kp.EXTRA_MODE_CASES, ids=kp.case_id)
def test_guard_fallback_agrees_with_exact(dcfm, K):
    c = kp.case(K)
    guard, exact = _run(dcfm, K, "guard_all")["states"], _run(dcfm, K, "exact")["states"]
    for it in range(1, kp.N_ITER + 1):
        bound = 2.0 * residual_rounding_bound(exact[it], c["Yd"]).T
        for f in ("ps", "omega"):
            e = scaled_rel_err(guard[it][f], exact[it][f], bound, TOL)
            print(f"K_PATHS_GUARD {kp.case_id(K)} guard_all vs exact iter {it}: {f} {e:.3e} (bound max {bound.max():.3e})")
            assert e < TOL, f"K = {K} iteration {it}: {f} of the guard's fallback vs the exact launch {e:.3e} (bar {TOL:.0e})"
