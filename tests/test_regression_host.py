"""CPU tests of the regression read-out (DCFM_FLAG_REGRESSION, dcfm_set_regression / dcfm_get_regression): the
panel restatement of csrc/regression.hip against the dense reference (the definition on the oracle's Sigma(s)) on
the oracle's own chain, for every shape and response set of the GPU sweep -- the bars of the GPU test are met by
the arithmetic alone; diagnostics.regression_summary and driver.unstandardize_regression."""
import functools

import numpy as np
import pytest

import precision_cases as qc
import probe_cases as pc
import regression_cases as gc
from helpers import rel_err


@functools.lru_cache(maxsize=None)
def _states(shape, rho):
    return qc.oracle_states(shape, rho=rho)


@pytest.mark.parametrize("which", gc.SETS)
@pytest.mark.parametrize("shape,rho", gc.CASES)
def test_panel_form_matches_the_dense_reference(shape, rho, which):
    """Bars: the project's normwise 1e-10 on all six moments, entrywise on coef the bound (1/S) sum_s
    4 (P + 2K + g) eps kappa_s sqrt(Theta(s)_aa C(s)_jj).  Measured: normwise <= 2.6e-13 (rho = 1), entrywise
    ratio <= 5.2e-4."""
    states = _states(shape, rho)
    assert len(states) == len(pc.SAVED)
    R = gc.response_set(shape[1], which)
    ref, got = gc.dense_ref(states, rho, R), gc.panel_ref(states, rho, R)
    errs = {f: rel_err(got[f], ref[f]) for f in gc.FIELDS}
    ratio = float(np.max(np.abs(got["coef"] - ref["coef"]) / ref["bound"]))
    print(f"{shape} rho={rho} {which} (q={R.size}): kappa max {max(ref['kappa']):.3e}, entrywise ratio {ratio:.3e}, "
          + ", ".join(f"{f} {e:.2e}" for f, e in errs.items()))
    assert all(e < 1e-10 for e in errs.values()), errs
    assert ratio <= 1.0
    assert not got["coef"][R].any() and not got["coef_m2"][R].any()
    assert np.array_equal(got["rcov"], got["rcov"].T)
    assert np.all(ref["r2"] > 0) and np.all(ref["r2"] < 1)


def test_the_mean_of_the_ratio_is_not_the_ratio_of_the_means():
    """What the feature is for: E[B(s)] differs from the plug-in -Theta_{.R} Theta_RR^-1 of the precision mean."""
    shape, rho = (30, 48, 4, 5), 0.5
    states = _states(shape, rho)
    R = gc.response_set(shape[1], "five")
    ref = gc.dense_ref(states, rho, R)
    Theta = sum(np.linalg.inv(pc.sample_sigma(st["Lambda"], st["omega"], rho)) for st in states) / len(states)
    plug = -Theta[:, R] @ np.linalg.inv(Theta[np.ix_(R, R)])
    plug[R] = 0.0
    gap = float(np.max(np.abs(ref["coef"] - plug)))
    print(f"max |E B - plug-in| = {gap:.3e}, bound max {ref['bound'].max():.3e}")
    assert gap > 1e3 * ref["bound"].max()


def test_regression_summary(dcfm):
    nan = np.nan
    coef = np.array([[0.5, 0.0], [-0.4, 0.3], [0.05, nan], [0.0, -0.2]])
    sd = np.array([[0.1, 0.0], [0.3, 0.0], [0.01, 0.1], [0.0, 0.05]])
    r = dcfm.regression_summary(coef, sd)
    z, sel = r["z"], r["selected"]
    assert z[0, 0] == 0.5 / 0.1 and z[1, 0] == pytest.approx(-0.4 / 0.3) and z[3, 1] == -0.2 / 0.05
    assert np.isposinf(z[1, 1]) and np.isnan(z[0, 1]) and np.isnan(z[2, 1]) and np.isnan(z[3, 0])
    assert np.array_equal(sel, np.array([[True, False], [False, True], [True, False], [False, True]]))
    assert [list(x) for x in r["predictors"]] == [[0, 2], [1, 3]]
    r1 = dcfm.diagnostics.regression_summary(coef[:, 0], sd[:, 0], z=1.0)
    assert r1["z"].shape == (4, 1) and list(r1["predictors"][0]) == [0, 2, 1]
    with pytest.raises(ValueError):
        dcfm.regression_summary(coef, sd[:3])


def test_unstandardize_regression(dcfm):
    """The coefficients of standardised columns against those of the raw columns, in closed form: ordinary least
    squares commutes with the columns' affine rescaling."""
    rng = np.random.default_rng(5)
    n, p_orig = 200, 9
    keep = np.array([0, 1, 2, 4, 5, 6, 8])                       # columns 3 and 7 were dropped
    varind = rng.permutation(keep.size)
    Y = rng.standard_normal((n, p_orig)) @ rng.standard_normal((p_orig, p_orig)) + rng.uniform(-3, 3, p_orig)
    Y[:, [3, 7]] = 0.0
    mean, sd = dcfm.column_moments(Y)
    cols = dcfm.output_columns(keep, varind)
    Z = (Y[:, cols] - mean[cols]) / sd[cols]
    R = np.array([4, 1])                                         # responses, Sigmaout's coordinates
    O = np.setdiff1d(np.arange(cols.size), R)
    S = np.cov(Z.T)
    coef = np.zeros((cols.size, 2))
    coef[O] = np.linalg.solve(S[np.ix_(O, O)], S[np.ix_(O, R)])
    C = S[np.ix_(R, R)] - S[np.ix_(R, O)] @ coef[O]
    reg = {"coef": coef, "coef_sd": np.abs(coef) / 3, "resid_cov": C, "resid_cov_sd": np.abs(C) / 5,
           "r2": 1 - C.diagonal(), "r2_sd": np.array([0.1, 0.2]), "count": 4, "responses": R}
    out = dcfm.unstandardize_regression(reg, mean, sd, keep, varind, p_orig)
    assert out["coef"].shape == out["coef_sd"].shape == (p_orig, 2) and out["count"] == 4
    assert np.array_equal(out["responses"], cols[R])
    # the raw-unit regression with an intercept
    So = np.cov(Y[:, cols].T)
    want = np.linalg.solve(So[np.ix_(O, O)], So[np.ix_(O, R)])
    assert np.allclose(out["coef"][cols[O]], want, rtol=1e-10, atol=1e-12)
    assert not out["coef"][cols[R]].any() and not out["coef"][[3, 7]].any()
    assert np.allclose(out["intercept"], mean[cols[R]] - mean[cols[O]] @ want, rtol=1e-10, atol=1e-12)
    assert np.allclose(out["resid_cov"], So[np.ix_(R, R)] - So[np.ix_(R, O)] @ want, rtol=1e-10, atol=1e-12)
    assert np.allclose(out["coef_sd"][cols], np.abs(out["coef"][cols]) / 3, rtol=1e-13, atol=0)
    assert np.array_equal(out["r2"], reg["r2"]) and np.array_equal(out["r2_sd"], reg["r2_sd"])
    assert np.all(np.isnan(dcfm.unstandardize_regression(reg, mean, sd, keep, varind, p_orig, fill=np.nan)["coef"][3]))
