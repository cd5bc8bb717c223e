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

The loading draw is also held, per row, to the diagonally scaled backward error (helpers.LoadingMeasure: the
residual and the system scaled by D = diag(Q_j)^-1/2), in all three modes: SBW_TOL_WELL = 8e-14 for rows with
cond(D Q_j D) <= 1e3, SBW_TOL = 7e-13 for the others, the class taken from the oracle's Q_j on the host.  Both bars
are 8 x what the reference itself reads (tests/test_loading_measure.py, CPU); neither comes from a device figure.
The normwise bar above is relative to ||Q_j|| ||lambda_j||, and at wide K ||Q_j|| is Plam's trailing diagonal
(tau_K ~ 2^K): a 1e-9 relative error in the data part of a wide factor does not move it.

test_flat_start_parity / test_flat_start_residual_modes: one iteration from k_paths.flat_start(K) (delta = 1,
tauh = 1, Plam = psi), burn-in 0, so that iteration is the one saved sample and Sigmaout is checked as above.  At
the default start the trailing 16 x 16 tiles of a factor with K >~ 65 are numerically diagonal (Plam up to 1e11),
so k_lambda_w's panel products, trailing updates and look-ahead steps beyond the first tiles multiply operands that
cannot change the answer; at the flat start every tile does (CPU: a 1e-9 plant in any one tile moves the measure
to >= 1.3e-11).  Same stage-wise assertions, every row's scaled measure <= SBW_TOL_WELL (cond(D Q_j D) <= 290),
Lambda forward against the oracle's draw from the device's own eta <= 1e-10 (cond(Q_j) <= 310), and the normwise
1e-13.  Never continued: a second iteration from the flat start is an excursion of the reference itself.

Measured on the MI355X: DESIGN.md section 2, "Every K-selected instantiation", with the outcome of 1e-9
perturbations of k_lambda<24>, k_lambda_w<128, 6> and k_lambda_w<128, 8> on scratch builds: K = 21, 23, 24 fail on
the first, K = 81, 88, 89, 96 on the second (81 and 89 by the scaled measure alone: 4.1e-11 and 5.1e-11 against
8e-14, where the normwise one reads 4e-22 and 1e-23), and the third, in the last row-panel's product, fails the
flat-start K = 113, 120, 121, 128 and nothing else.
"""
import functools

import numpy as np
import pytest

import k_paths as kp
from helpers import (SBW_TOL_WELL, as_oracle_state, loading_scaled_bars, rel_err, residual_rounding_bound,
                     scaled_rel_err, stacked_draws, stagewise_errors, state_dict)
from oracle import dc_oracle as F

pytestmark = pytest.mark.gpu

TOL = 1e-10           # the project's stage-wise bar
BW_TOL = 1e-13        # loading backward error
SIGMA_TOL = 1e-12     # Sigmaout against the host sum of the device's own samples
FLAT_FWD_TOL = 1e-10  # Lambda forward against the oracle at the flat start (cond(Q_j) <= 310)


def _plan(flat):
    """(burn-in, mcmc, thin, iterations) of the default-start chain or of the flat start's one iteration."""
    if flat:
        return kp.FLAT_BURNIN, kp.FLAT_MCMC, kp.FLAT_THIN, 1
    return kp.BURNIN, kp.MCMC, kp.THIN, kp.N_ITER


@functools.lru_cache(maxsize=None)
def _run(dcfm, K, mode, flat=False, cases=kp):
    """The chain of case K in `mode`, one iteration per call: the states (the start first), Sigmaout and the
    saved-sample count.  Made once, shared, read only.  `flat`: k_paths.flat_case, exactly one iteration.
    `cases`: the case list's module (case, shape, case_id, MODES and the same 3-iteration plan): k_paths, keyed by
    K, or tests/tiny_shapes.py, keyed by (n, P, g, K)."""
    c = cases.flat_case(K) if flat else cases.case(K)
    n, P, g, Kf = cases.shape(K)
    burnin, mcmc, thin, n_iter = _plan(flat)
    assert flat or (cases.BURNIN, cases.MCMC, cases.THIN, cases.N_ITER) == (burnin, mcmc, thin, n_iter)
    start = state_dict(c["st"])
    smp = dcfm.Sampler(n, P, g, Kf, c["rho"], burnin, mcmc, thin, inject_draws=True, flags=cases.MODES[mode])
    try:
        smp.set_data(c["Yd"])
        smp.set_state({f: v for f, v in start.items() if f != "eta"})
        smp.set_draws(stacked_draws(c["src"], 1, n_iter), 1, n_iter)
        states = [{f: np.array(v) for f, v in start.items()}]
        for it in range(1, n_iter + 1):
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


def _check(dcfm, K, mode, flat=False, cases=kp):
    c = cases.flat_case(K) if flat else cases.case(K)
    r = _run(dcfm, K, mode, flat, cases)
    burnin, mcmc, thin, n_iter = _plan(flat)
    tag = ("K_PATHS_FLAT" if flat else "K_PATHS") if cases is kp else "TINY_SHAPES"
    states = r["states"]
    assert len(states) == n_iter + 1
    worst = {}
    for it in range(1, n_iter + 1):
        got = states[it]
        errs, bw, ref, (sbw, cond) = stagewise_errors(as_oracle_state(states[it - 1]), got, c["Yd"], c["rho"],
                                                      c["hyper"], c["src"].iteration(it), scaled=True)
        bound = residual_rounding_bound(got, c["Yd"]).T            # P x g, the ps / omega layout
        for f in ("ps", "omega"):
            worst[f + "_raw"] = max(worst.get(f + "_raw", 0.0), errs[f])
            errs[f] = scaled_rel_err(got[f], getattr(ref, f), bound, TOL)
        worst["ps_bound_max"] = max(worst.get("ps_bound_max", 0.0), float(bound.max()))
        worst["lambda_bw"] = max(worst.get("lambda_bw", 0.0), bw)
        for f, e in errs.items():
            worst[f] = max(worst.get(f, 0.0), e)
        # the scaled measure, every row against the bar of its class (cond of the oracle's Q_j, on the host)
        bars = np.full(cond.shape, SBW_TOL_WELL) if flat else loading_scaled_bars(cond)
        at = np.unravel_index(np.argmax(sbw / bars), sbw.shape)
        well = bars == SBW_TOL_WELL
        worst["lambda_sbw"] = max(worst.get("lambda_sbw", 0.0), float(sbw.max()))
        worst["lambda_sbw_over_bar"] = max(worst.get("lambda_sbw_over_bar", 0.0), float(sbw[at] / bars[at]))
        worst["lambda_sbw_well"] = max(worst.get("lambda_sbw_well", 0.0), float(sbw[well].max()) if well.any() else 0.0)
        worst["cond_dqd"] = max(worst.get("cond_dqd", 0.0), float(cond.max()))
        print(f"{tag} {cases.case_id(K)} {mode} iter {it}:", {f: f"{e:.2e}" for f, e in sorted(errs.items())},
              f"lambda_bw {bw:.2e} lambda_sbw {sbw.max():.2e} (worst against its bar: {sbw[at]:.2e} at shard {at[0]} row "
              f"{at[1]}, cond(DQD) {cond[at]:.2e}, bar {bars[at]:.0e}; {int((~well).sum())} of {well.size} rows over "
              f"cond 1e3, cond(DQD) <= {cond.max():.2e})")
        for f, e in errs.items():
            assert e < TOL, f"K = {K} {mode} iteration {it}: stage {f} rel err {e:.3e} (bar {TOL:.0e})"
        assert bw <= BW_TOL, f"K = {K} {mode} iteration {it}: loading backward error {bw:.3e} (bar {BW_TOL:.0e})"
        assert sbw[at] <= bars[at], (f"K = {K} {mode} iteration {it}: scaled loading backward error {sbw[at]:.3e} at shard "
                                     f"{at[0]} row {at[1]} (cond(DQD) {cond[at]:.3e}, bar {bars[at]:.0e})")
        if flat:
            # cond(Q_j) <= 310 here, so a forward bar on Lambda is legitimate: the oracle's draw from got's own eta
            fwd = rel_err(got["Lambda"], _oracle_lambda(states[it - 1], got, c, it))
            worst["lambda_fwd"] = fwd
            print(f"{tag} {cases.case_id(K)} {mode}: Lambda forward {fwd:.2e}")
            assert fwd <= FLAT_FWD_TOL, f"flat K = {K} {mode}: Lambda against the oracle's {fwd:.3e} (bar {FLAT_FWD_TOL:.0e})"
    # Sigmaout (dc:180-195) from the device's own saved states
    S = r["sigma"]
    assert r["saved"] == mcmc // thin == (1 if flat else 2)
    assert np.all(np.isfinite(S)) and np.array_equal(S, S.T), "Sigmaout not exactly symmetric"
    saved = [it for it in range(1, n_iter + 1) if it % thin == 0 and it > burnin]
    want = sum(F.assemble_sample(as_oracle_state(states[it]), c["rho"]) for it in saved) / (mcmc / thin)
    worst["sigma"] = float(np.max(np.abs(S - want)) / np.max(np.abs(want)))
    print(f"{tag}_WORST {cases.case_id(K)} {mode} classes {kp.classes(cases.shape(K)[3])} shape {cases.shape(K)}:",
          {f: f"{e:.2e}" for f, e in sorted(worst.items())})
    assert worst["sigma"] < SIGMA_TOL, f"K = {K} {mode}: Sigmaout vs the device's own samples {worst['sigma']:.3e}"
    return worst


def _oracle_lambda(before, got, c, it):
    """The vectorised oracle's loading draw (P x K x g) of iteration `it` from the state `before`, with got's
    own X, Z and eta: what helpers.stagewise_errors builds its systems from."""
    from oracle import vectorised as V
    D = V._as_data(c["Yd"])
    st = as_oracle_state(before)
    for f in ("X", "Z", "eta"):
        getattr(st, f)[...] = np.asarray(got[f], dtype=np.float64).reshape(getattr(st, f).shape)
    _, _, _, b, L, z = V.loading_systems(st, D, c["src"].iteration(it))
    return np.moveaxis(V._loading_solve(L, b, z), 0, 2)


@pytest.mark.parametrize("K", kp.CASES, ids=kp.case_id)
def test_stagewise_parity(dcfm, K, record_property):
    for f, e in _check(dcfm, K, "default").items():
        record_property(f"worst_{f}", e)


@pytest.mark.parametrize("mode", ["guard_all", "exact"])
@pytest.mark.parametrize("K", kp.EXTRA_MODE_CASES, ids=kp.case_id)
def test_stagewise_parity_residual_modes(dcfm, K, mode, record_property):
    for f, e in _check(dcfm, K, mode).items():
        record_property(f"worst_{f}", e)


@pytest.mark.parametrize("K", kp.FLAT_CASES, ids=kp.case_id)
def test_flat_start_parity(dcfm, K, record_property):
    """One iteration from k_paths.flat_start(K) (delta = 1, tauh = 1, Plam = psi), where every 16 x 16 tile of the
    factor changes the answer (tests/test_loading_measure.py::test_flat_start_reaches_every_tile).  _check's
    stage-wise assertions and Sigmaout (burn-in 0, one saved sample), every row of the scaled measure against
    SBW_TOL_WELL, and Lambda forward against the oracle <= 1e-10."""
    for f, e in _check(dcfm, K, "default", flat=True).items():
        record_property(f"worst_{f}", e)


@pytest.mark.parametrize("mode", ["guard_all", "exact"])
@pytest.mark.parametrize("K", kp.FLAT_MODE_CASES, ids=kp.case_id)
def test_flat_start_residual_modes(dcfm, K, mode, record_property):
    for f, e in _check(dcfm, K, mode, flat=True).items():
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
