"""CPU tests of the log-likelihood draws' mathematics: the NumPy restatement of the recursion
(loglik_cases.recursion, what csrc/loglik.hip computes) against the dense solve and slogdet of the oracle's
Sigma(s) on the oracle's saved states of the injected chains the GPU tests run, within the bounds the GPU
tests use, and diagnostics.waic against values worked out by hand."""
import numpy as np
import pytest

import loglik_cases as lc
import precision_cases as qc
from helpers import make_case


@pytest.mark.parametrize("shape,rho", lc.HOST_SHAPES)
def test_recursion_matches_the_dense_solve(shape, rho):
    n, p, g, K = shape
    seed = 23 if shape == (60, 400, 4, 5) else 21                # the loopback case's chain
    Yd = make_case(n, p, g, K, seed=seed, k0=4, rho=rho)["Yd"]
    for s, st in enumerate(qc.oracle_states(shape, rho=rho, case_seed=seed)):
        q, ld = lc.recursion(Yd, st["Lambda"], st["omega"], rho)
        assert q.shape == (n,) and np.all(q > 0)
        lc.assert_draw(q, ld, Yd, st, rho, f"{shape} rho={rho} state {s}")


def test_waic_by_hand(dcfm):
    """Three samples, two points.  Point 0: ll = (-1, -2, -3): mean density (e^-1 + e^-2 + e^-3) / 3, variance
    1.  Point 1: ll = (-4, -4, -7): lppd = -4 + log((2 + e^-3) / 3), mean -5, variance (1 + 1 + 4) / 2 = 3."""
    ll = np.array([[-1.0, -4.0], [-2.0, -4.0], [-3.0, -7.0]])
    r = dcfm.waic(ll)
    lppd = np.array([np.log((np.exp(-1.0) + np.exp(-2.0) + np.exp(-3.0)) / 3.0), -4.0 + np.log((2.0 + np.exp(-3.0)) / 3.0)])
    pw = np.array([1.0, 3.0])
    assert r["lppd_i"] == pytest.approx(lppd, rel=1e-15) and r["p_waic_i"] == pytest.approx(pw, rel=1e-15)
    assert r["elpd_i"] == pytest.approx(lppd - pw, rel=1e-15)
    assert r["lppd"] == pytest.approx(lppd.sum(), rel=1e-15) and r["p_waic"] == pytest.approx(4.0, rel=1e-15)
    assert r["elpd_waic"] == pytest.approx((lppd - pw).sum(), rel=1e-15)
    assert r["waic"] == pytest.approx(-2.0 * (lppd - pw).sum(), rel=1e-15)
    e = lppd - pw                                                 # n var_i with ddof = 1, n = 2: (e0 - e1)^2
    assert r["se"] == pytest.approx(abs(e[0] - e[1]), rel=1e-14)
    assert set(r) == {"lppd_i", "p_waic_i", "elpd_i", "lppd", "p_waic", "elpd_waic", "waic", "se"}
    # far below the underflow of exp: the shift keeps the log-mean-exp finite
    r2 = dcfm.waic(np.array([[-2000.0], [-2001.0]]))
    assert r2["lppd_i"][0] == pytest.approx(-2000.0 + np.log((1.0 + np.exp(-1.0)) / 2.0), rel=1e-15)


def test_waic_constant_rows(dcfm):
    r = dcfm.waic(np.full((4, 3), -2.5))
    assert np.array_equal(r["p_waic_i"], np.zeros(3)) and np.array_equal(r["lppd_i"], np.full(3, -2.5))
    assert r["p_waic"] == 0.0 and r["lppd"] == -7.5 and r["waic"] == 15.0 and r["se"] == 0.0


def test_waic_minus_infinity_column(dcfm):
    ll = np.array([[-1.0, -np.inf, -4.0], [-2.0, -np.inf, -4.0], [-3.0, -np.inf, -7.0]])
    r = dcfm.waic(ll)
    ok = dcfm.waic(ll[:, [0, 2]])
    for f in ("lppd_i", "p_waic_i", "elpd_i"):
        assert np.array_equal(r[f][[0, 2]], ok[f]) and np.all(np.isfinite(r[f][[0, 2]]))
    assert r["lppd_i"][1] == -np.inf


def test_waic_needs_two_samples(dcfm):
    for bad in (np.zeros((1, 5)), np.zeros(5), np.zeros((0, 5)), np.zeros((2, 3, 4))):
        with pytest.raises(ValueError):
            dcfm.waic(bad)
