"""CPU tests of the precision draws' mathematics: the NumPy restatement of the nested Woodbury recursion
(precision_cases.woodbury, what csrc/precision.hip computes) against a dense solve and slogdet of the
oracle's Sigma(s) on random (Lambda, omega, rho) -- rho = 0 and rho = 1, K > P and g = 1 included -- within
a quarter of the bounds the GPU tests use, and diagnostics.heldout_log_density against values worked out
by hand."""
import numpy as np
import pytest

import precision_cases as qc

# (P, K, g, nv, rho)
CASES = [(20, 3, 3, 5, 0.5), (20, 3, 3, 5, 0.0), (20, 3, 3, 5, 1.0), (7, 11, 2, 4, 0.3), (21, 1, 1, 3, 0.9),
         (37, 5, 2, 32, 0.5), (9, 4, 5, 0, 0.5), (50, 40, 2, 6, 0.999)]


@pytest.mark.parametrize("P,K,g,nv,rho", CASES)
def test_recursion_matches_the_dense_solve(P, K, g, nv, rho):
    rng = np.random.default_rng(100 * P + K)
    Lam = rng.standard_normal((P, K, g))
    om = rng.gamma(2.0, 0.5, (P, g)) + 0.05
    V = rng.standard_normal((P * g, nv))
    if nv >= 3:
        V[:, 1] = 0.0
    Q, ld = qc.woodbury(V, Lam, om, rho)
    rq, rl, kappa = qc.ratios(Q, ld, V, {"Lambda": Lam, "omega": om}, rho)
    print(f"P={P} K={K} g={g} nv={nv} rho={rho}: kappa {kappa:.3e}, Q err / bound {rq:.4f}, log det err / bound {rl:.5f}")
    assert kappa <= 1e6 and rq <= 0.25 and rl <= 0.25
    assert Q.shape == (nv, nv) and np.isfinite(ld)
    if nv >= 3:                                              # the all-zero probe: exact zeros
        assert not Q[1].any() and not Q[:, 1].any()


def test_heldout_log_density_by_hand(dcfm):
    """Two samples, one probe, p = 2: log det (0, 2 log 2), quadratic forms (1, 3).  The per-sample log
    densities are -(2 log 2 pi + 0 + 1) / 2 and -(2 log 2 pi + 2 log 2 + 3) / 2 = the first - log 2 - 1, so
    the densities are d and d / (2 e) and lppd = log d + log((1 + 1 / (2 e)) / 2)."""
    Q = np.array([[[1.0]], [[3.0]]])
    ld = np.array([0.0, 2.0 * np.log(2.0)])
    r = dcfm.heldout_log_density(Q, ld, 2)
    l0 = -np.log(2.0 * np.pi) - 0.5
    assert r["per_sample"].shape == (2, 1)
    assert r["per_sample"][:, 0] == pytest.approx([l0, l0 - np.log(2.0) - 1.0], rel=1e-15)
    want = l0 + np.log((1.0 + 0.5 / np.e) / 2.0)
    assert r["lppd"].shape == (1,) and r["lppd"][0] == pytest.approx(want, rel=1e-15)
    assert r["total"] == pytest.approx(want, rel=1e-15)
    # two probes, densities far below the underflow of exp: the shift keeps the log-mean-exp finite
    Q2 = np.zeros((2, 2, 2))
    Q2[:, 0, 0] = [4000.0, 4002.0]
    Q2[:, 1, 1] = [2.0, 2.0]
    r2 = dcfm.heldout_log_density(Q2, np.zeros(2), 1)
    c = -0.5 * np.log(2.0 * np.pi)
    assert r2["lppd"][0] == pytest.approx(c - 2000.0 + np.log((1.0 + np.exp(-1.0)) / 2.0), rel=1e-15)
    assert r2["lppd"][1] == pytest.approx(c - 1.0, rel=1e-15) and r2["total"] == pytest.approx(r2["lppd"].sum())
    assert dcfm.heldout_log_density(np.zeros((3, 0, 0)), np.zeros(3), 5)["lppd"].shape == (0,)
    with pytest.raises(ValueError):
        dcfm.heldout_log_density(np.zeros((2, 1, 1)), np.zeros(3), 2)
