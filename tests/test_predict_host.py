"""CPU tests of the conditional prediction's mathematics: the NumPy restatement of the recursion
(predict_cases.recursion, what csrc/predict.hip computes) against the dense Gaussian conditional of the oracle's
Sigma(s) on the oracle's saved states of the chains the GPU tests run -- rho in {0, 0.3, 0.5, 0.9, 1}, K > P and
g = 1, every mask kind -- on every row for yhat, cv, q and log det, within a quarter of the bounds the GPU tests
use."""
import functools

import numpy as np
import pytest

import precision_cases as qc
import predict_cases as dc

BASE = (30, 60, 3, 3)
# (shape, rho, mask kind)
CASES = ([(BASE, rho, "random") for rho in (0.0, 0.3, 0.5, 0.9, 1.0)] +
         [(BASE, 0.5, kind) for kind in dc.MASKS if kind != "random"] +
         [((30, 14, 2, 11), 0.5, "random"), ((30, 14, 2, 11), 0.3, "shard_off"), ((30, 21, 1, 1), 0.5, "random"),
          ((30, 21, 1, 1), 0.9, "single")])


@functools.lru_cache(maxsize=None)
def _states(shape, rho):
    return qc.oracle_states(shape, rho=rho)


@pytest.mark.parametrize("shape,rho,kind", CASES)
def test_recursion_matches_the_dense_conditional(shape, rho, kind):
    n, p, g, K = shape
    P, T = p // g, 5
    ob, Y = dc.mask(kind, P, g), dc.new_rows(p, T)
    Ynan = np.where(ob[:, None] != 0, Y, np.nan)              # unobserved entries are ignored
    worst = {}
    for st in _states(shape, rho):
        yhat, cv, q, ld = dc.recursion(Ynan, ob, st["Lambda"], st["omega"], rho)
        d = dc.dense(Y, ob, st["Lambda"], st["omega"], rho)
        r = dc.ratios(yhat, cv, q, ld, d, dc.bounds(d, P, K, g, T))
        assert d["kappa"] <= 1e6
        for f, v in r.items():
            worst[f] = max(worst.get(f, 0.0), v)
        assert np.isfinite(yhat).all() and np.isfinite(cv).all() and (cv > 0).all()
        assert not yhat[:, 1].any() and q[1] == 0.0           # the all-zero new row: exact zeros
        # observed rows: the signal's conditional mean plus omega_j (Sigma_AA^-1 y)_j gives y_j back (dense side)
        om = st["omega"].T.reshape(-1)
        A = ob != 0
        scale = np.abs(Y[A]).max() if A.any() else 0.0
        assert np.all(np.abs(d["yhat"][A] + om[A, None] * d["z"][A] - Y[A]) <= 64 * p * dc.EPS * d["kappa"] * max(scale, 1.0))
        if kind == "empty":
            assert not yhat.any() and not q.any() and abs(ld) <= 0.0
            assert np.all(np.abs(cv - d["diag"]) <= 4 * (P + K + g) * dc.EPS * d["diag"])
    print(f"{shape} rho={rho} {kind}: err / bound " + ", ".join(f"{f} {v:.4f}" for f, v in worst.items()))
    assert all(v <= 0.25 for v in worst.values()), worst


def test_law_of_total_variance_accumulators():
    """Running: the averages it forms are those of the per-sample dense values."""
    st = _states(BASE, 0.5)
    P, g, K = 20, 3, 3
    ob, Y = dc.mask("random", P, g), dc.new_rows(60, 2)
    run, ys, cvs = dc.Running(), [], []
    for s in st:
        d = dc.dense(Y, ob, s["Lambda"], s["omega"], 0.5)
        run.add(d, dc.bounds(d, P, K, g, 2))
        ys.append(d["yhat"])
        cvs.append(d["cv"])
    r = run.ratios(np.mean(ys, axis=0), np.mean(np.square(ys), axis=0), np.mean(cvs, axis=0))
    assert run.n == len(st) and all(v <= 1.0 for v in r.values()), r
