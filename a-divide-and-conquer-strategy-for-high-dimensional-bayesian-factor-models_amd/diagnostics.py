"""Convergence diagnostics across chains on the per-iteration chain
trace the device records (``Sampler.set_trace`` / dcfm_set_trace).

The reference runs one chain and keeps no trace (divideconquer.m:180-196 accumulates only
Sigmaout); config c4 runs 8 parallel chains (BASELINE configs[3]), so the build adds the
standard between/within-chain checks on scalar summaries of each chain's state:

* ``split_rhat`` — potential scale reduction factor on split chains (Gelman et al.,
  Bayesian Data Analysis 3rd ed., §11.4): each chain is cut in halves, and
  R = sqrt(((n-1)/n W + B/n) / W) with B, W the between / within variances of the halves.
* ``ess`` — effective sample size over all chains (BDA3 §11.5: combined autocorrelation
  from the variogram, summed over Geyer's initial positive sequence of lag pairs).

Inputs are arrays of shape (chains, iterations) or (chains, iterations, quantities).
"""
from __future__ import annotations

import numpy as np

TRACE_FIELDS = ("lambda_fro2", "tr_omega", "sum_log_ps", "sum_log_tau")


def _as3(x):
    x = np.asarray(x, dtype=np.float64)
    if x.ndim == 2:
        x = x[:, :, None]
    if x.ndim != 3:
        raise ValueError("traces must be (chains, iterations[, quantities])")
    return x


def _split(x):
    n = x.shape[1] // 2
    if n < 2:
        raise ValueError("need at least 4 iterations per chain")
    return np.concatenate([x[:, :n], x[:, x.shape[1] - n:]], axis=0)     # (2m, n, q)


def split_rhat(traces) -> np.ndarray:
    """Split-R-hat per quantity (BDA3 §11.4); values near 1 mean the chains mix."""
    x = _split(_as3(traces))
    n = x.shape[1]
    means = x.mean(axis=1)                                  # (2m, q)
    B = n * means.var(axis=0, ddof=1)
    W = x.var(axis=1, ddof=1).mean(axis=0)
    var_plus = (n - 1) / n * W + B / n
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.sqrt(var_plus / W)


def ess(traces) -> np.ndarray:
    """Effective sample size per quantity over all split chains (BDA3 §11.5)."""
    x = _split(_as3(traces))
    m, n, q = x.shape
    means = x.mean(axis=1)
    B = n * means.var(axis=0, ddof=1)
    W = x.var(axis=1, ddof=1).mean(axis=0)
    var_plus = (n - 1) / n * W + B / n
    out = np.empty(q)
    for k in range(q):
        if not var_plus[k] > 0:
            out[k] = np.nan
            continue
        rho = []
        for t in range(1, n):
            vt = np.mean((x[:, t:, k] - x[:, :-t, k]) ** 2)          # variogram V_t
            rho.append(1.0 - vt / (2.0 * var_plus[k]))
        # Geyer: sum pairs rho_{2s-1} + rho_{2s} while they stay positive (rho_0 = 1 first)
        r = np.concatenate([[1.0], np.asarray(rho)])
        total = 0.0
        for s in range(0, len(r) - 1, 2):
            pair = r[s] + r[s + 1]
            if pair < 0:
                break
            total += pair
        out[k] = m * n / max(2.0 * total - 1.0, 1e-12)
    return out


def summarize(traces, fields=TRACE_FIELDS) -> dict:
    """{field: {"rhat": R, "ess": E}} for a (chains, iterations, 4) device trace."""
    r, e = split_rhat(traces), ess(traces)
    return {f: {"rhat": float(r[i]), "ess": float(e[i])} for i, f in enumerate(fields)}


def summarize_probes(draws, q=(0.025, 0.5, 0.975)) -> dict:
    """Posterior summaries of the per-sample probe draws ``Q[s] = V' Sigma(s) V`` (``Sampler.probe_draws``,
    shape (S, nv, nv); a single (nv, nv) draw is taken as S = 1).  Returns ``mean`` and ``sd`` (nv x nv, over
    the draws; sd in the population form), ``quantiles`` (len(q), nv, nv) at the levels ``q`` (NumPy's
    default linear interpolation), ``corr`` (S, nv, nv), the correlation matrix of every draw
    ``Q_ab / sqrt(Q_aa Q_bb)`` -- a nonlinear functional, so it is formed per draw and not from the mean;
    NaN where a probe's variance is not positive, e.g. an all-zero probe -- and ``corr_quantiles``
    (len(q), nv, nv).  Contrasts, variance ratios and other functionals follow the same way from
    ``draws``.  The precision draws ``V' Sigma(s)^-1 V`` of ``Sampler.precision_draws`` have the same shape
    and go through unchanged (``corr`` is then the partial-correlation-like ratio of the projected precision)."""
    Q = np.asarray(draws, dtype=np.float64)
    if Q.ndim == 2:
        Q = Q[None]
    if Q.ndim != 3 or Q.shape[1] != Q.shape[2] or Q.shape[0] < 1:
        raise ValueError(f"draws must be (S, nv, nv) with S >= 1, got {Q.shape}")
    qs = np.asarray(q, dtype=np.float64).reshape(-1)
    d = np.diagonal(Q, axis1=1, axis2=2)                        # (S, nv) variances of the projections
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.sqrt(np.where(d > 0, d, np.nan))
        corr = Q / (s[:, :, None] * s[:, None, :])
    return {"mean": Q.mean(axis=0), "sd": Q.std(axis=0), "quantiles": np.quantile(Q, qs, axis=0),
            "corr": corr, "corr_quantiles": np.quantile(corr, qs, axis=0), "q": qs}


def heldout_log_density(Q, logdet, p) -> dict:
    """Held-out Gaussian log density from the precision draws (``Sampler.precision_draws``): with
    ``Q[s] = V' Sigma(s)^-1 V`` (S, nv, nv), ``logdet[s] = log det Sigma(s)`` (S,) and every column of V one
    centred, standardised held-out row in Sigmaout's coordinates (p entries), returns ``per_sample``
    (S, nv), ``-(p log 2 pi + logdet[s] + Q[s, c, c]) / 2``, the log density of row c under sample s;
    ``lppd`` (nv,), the log of the mean over s of the densities (log-mean-exp, shifted by the maximum so
    that it neither overflows nor underflows) -- the log pointwise predictive density, by which ``k``,
    ``g`` and ``rho`` can be compared on held-out rows -- and ``total``, the sum of lppd.  Standardised
    units: a density in the original units subtracts ``sum(log sd)``."""
    Q = np.asarray(Q, dtype=np.float64)
    ld = np.asarray(logdet, dtype=np.float64).reshape(-1)
    if Q.ndim != 3 or Q.shape[1] != Q.shape[2] or Q.shape[0] < 1 or ld.shape[0] != Q.shape[0]:
        raise ValueError(f"Q must be (S, nv, nv) and logdet (S,) with S >= 1, got {Q.shape} and {ld.shape}")
    per = -0.5 * (p * np.log(2.0 * np.pi) + ld[:, None] + np.diagonal(Q, axis1=1, axis2=2))
    top = per.max(axis=0)
    safe = np.where(np.isfinite(top), top, 0.0)
    with np.errstate(divide="ignore"):
        lppd = safe + np.log(np.mean(np.exp(per - safe), axis=0))
    return {"per_sample": per, "lppd": lppd, "total": float(lppd.sum())}


def conditional_log_density(maha, logdet, n_obs) -> dict:
    """Log density of partly observed rows from the conditional prediction's draws (``Sampler.predict``): with
    ``maha[s, t] = y_A' Sigma_AA(s)^-1 y_A`` (S, nt) of new row t, ``logdet[s] = log det Sigma_AA(s)`` (S,) and
    ``n_obs = |A|`` the number of observed variables, returns ``per_sample`` (S, nt),
    ``-(n_obs log 2 pi + logdet[s] + maha[s, t]) / 2``, the log density of the observed part of row t under
    sample s; ``lppd`` (nt,), the log of the mean over s of the densities (log-mean-exp, shifted by the maximum
    as in ``heldout_log_density``), and ``total``, the sum of lppd.  The units are standardised (the
    coordinates the sweep works in): a density in the data's units subtracts ``sum_{j in A} log sd_j``, sd the
    training columns' standard deviations."""
    q = np.asarray(maha, dtype=np.float64)
    ld = np.asarray(logdet, dtype=np.float64).reshape(-1)
    if q.ndim == 1:
        q = q[:, None]
    if q.ndim != 2 or q.shape[0] < 1 or ld.shape[0] != q.shape[0]:
        raise ValueError(f"maha must be (S, nt) and logdet (S,) with S >= 1, got {q.shape} and {ld.shape}")
    per = -0.5 * (float(n_obs) * np.log(2.0 * np.pi) + ld[:, None] + q)
    if per.shape[1] == 0:
        return {"per_sample": per, "lppd": np.zeros(0), "total": 0.0}
    top = per.max(axis=0)
    safe = np.where(np.isfinite(top), top, 0.0)
    with np.errstate(divide="ignore"):
        lppd = safe + np.log(np.mean(np.exp(per - safe), axis=0))
    return {"per_sample": per, "lppd": lppd, "total": float(lppd.sum())}


def waic(ll) -> dict:
    """WAIC (Watanabe 2010; Gelman, Hwang and Vehtari 2014) from the pointwise log-likelihood draws ``ll`` of
    shape (S, n), S >= 2 saved samples by n training rows (``Sampler.loglik_draws``).  Per point: ``lppd_i``,
    the log of the mean over s of the densities (log-mean-exp, shifted by the maximum as in
    ``heldout_log_density``), ``p_waic_i``, the sample variance of ll over s (ddof = 1), and
    ``elpd_i = lppd_i - p_waic_i``.  Totals: ``lppd``, ``p_waic`` (the effective number of parameters),
    ``elpd_waic``, ``waic = -2 elpd_waic`` and ``se = sqrt(n var_i(elpd_i))`` (ddof = 1), the standard error of elpd_waic.
    The units are standardised (the data the sweep holds): a density in the original units subtracts
    ``sum(log sd)`` over the kept columns from every ll[s, i].  Chains that are compared (over g, k, rho) must
    use the same Y.  A ``p_waic_i`` above 0.4 is the usual warning sign that WAIC is unreliable for that point
    (Vehtari, Gelman and Gabry 2017); PSIS-LOO takes the same ``ll``."""
    ll = np.asarray(ll, dtype=np.float64)
    if ll.ndim != 2 or ll.shape[0] < 2:
        raise ValueError(f"ll must be (S, n) with S >= 2, got {ll.shape}")
    n = ll.shape[1]
    top = ll.max(axis=0)
    safe = np.where(np.isfinite(top), top, 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        lppd_i = safe + np.log(np.mean(np.exp(ll - safe), axis=0))
        p_i = ll.var(axis=0, ddof=1)
    elpd_i = lppd_i - p_i
    elpd = float(elpd_i.sum())
    with np.errstate(invalid="ignore"):
        se = float(np.sqrt(n * elpd_i.var(ddof=1))) if n > 1 else 0.0   # var over the points with ddof = 1
    return {"lppd_i": lppd_i, "p_waic_i": p_i, "elpd_i": elpd_i, "lppd": float(lppd_i.sum()),
            "p_waic": float(p_i.sum()), "elpd_waic": elpd, "waic": -2.0 * elpd, "se": se}


def partial_correlations(T) -> np.ndarray:
    """Partial correlations from a precision matrix T (``Sampler.get_precision_mean``, or any symmetric
    p x p precision): ``-T_ab / sqrt(T_aa T_bb)`` off the diagonal, the correlation of variables a and b
    given all the others, with a unit diagonal.  NaN in the rows and columns whose diagonal entry is not
    positive."""
    T = np.asarray(T, dtype=np.float64)
    if T.ndim != 2 or T.shape[0] != T.shape[1]:
        raise ValueError(f"T must be p x p, got {T.shape}")
    d = T.diagonal()
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.sqrt(np.where(d > 0, d, np.nan))
        R = -T / (s[:, None] * s[None, :])
    R[np.diag_indices_from(R)] = np.where(d > 0, 1.0, np.nan)
    return R


def correlation(S) -> np.ndarray:
    """The plug-in correlation matrix of a covariance S (``Sampler.get_sigma``, or any symmetric p x p
    covariance): ``S_ab / sqrt(S_aa S_bb)`` with an exact unit diagonal; NaN in the rows and columns whose
    diagonal entry is not positive.  The precision side's counterpart is ``partial_correlations(T)``.  Of
    Sigmaout it is the correlation of the posterior mean covariance, not the posterior mean of the per-sample
    correlation (``Sampler.get_corr("mean")``), and it carries no uncertainty."""
    S = np.asarray(S, dtype=np.float64)
    if S.ndim != 2 or S.shape[0] != S.shape[1]:
        raise ValueError(f"S must be p x p, got {S.shape}")
    d = S.diagonal()
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.sqrt(np.where(d > 0, d, np.nan))
        R = S / (s[:, None] * s[None, :])
    R[np.diag_indices_from(R)] = np.where(d > 0, 1.0, np.nan)
    return R


def partial_correlation_edges(mean, sd, z=1.96, min_abs=0.0) -> dict:
    """Edges of the graphical model from the posterior mean and standard deviation of the partial
    correlations (``Sampler.get_partial_corr("mean")`` / ``("sd")``, or ``divideconquer(..., return_partial=True)``).
    It works on any (mean, sd) pair of p x p matrices: given ``Sampler.get_corr("mean")`` / ``("sd")`` (or
    ``divideconquer(..., return_corr=True)``) it thresholds the marginal correlations, the edges of a
    co-expression network, the same way.
    Returns ``{"z": |mean| / sd, "edges": bool p x p}``: ``z`` is inf where sd == 0 and mean != 0, and NaN where
    either input is NaN or both are 0; ``edges[a, b]`` holds where ``|mean| >= min_abs`` and ``z-score >= z``
    on the pair (a, b) *and* on (b, a), so it is symmetric; its diagonal is False, and a NaN is no edge."""
    mean, sd = np.asarray(mean, dtype=np.float64), np.asarray(sd, dtype=np.float64)
    if mean.ndim != 2 or mean.shape[0] != mean.shape[1] or sd.shape != mean.shape:
        raise ValueError(f"mean and sd must both be p x p, got {mean.shape} and {sd.shape}")
    with np.errstate(divide="ignore", invalid="ignore"):
        zs = np.abs(mean) / sd
        e = (np.abs(mean) >= min_abs) & (zs >= z)
    e = e & e.T
    e[np.diag_indices_from(e)] = False
    return {"z": zs, "edges": e}


def regression_summary(coef, coef_sd, z=1.96) -> dict:
    """Selected predictors of a factor regression from the posterior mean and standard deviation of its
    coefficients (``Sampler.regression()``'s ``coef`` / ``coef_sd``, or ``divideconquer(..., regress=cols)``), both
    (p, q), one column per response.  Returns ``{"z": mean / sd (signed), "selected": bool (p, q), "predictors":
    a list of q index arrays}``: ``z`` is +-inf where sd == 0 and mean != 0 and NaN where either input is NaN or
    both are 0 (the rows of the responses and of dropped columns); ``selected[a, j]`` holds where ``|z| >= z``,
    a NaN selects nothing, and ``predictors[j]`` lists the selected rows of response j by decreasing ``|z|``."""
    coef, coef_sd = np.asarray(coef, dtype=np.float64), np.asarray(coef_sd, dtype=np.float64)
    if coef.ndim == 1:
        coef, coef_sd = coef[:, None], coef_sd.reshape(-1, 1)
    if coef.ndim != 2 or coef_sd.shape != coef.shape:
        raise ValueError(f"coef and coef_sd must both be (p, q), got {coef.shape} and {coef_sd.shape}")
    with np.errstate(divide="ignore", invalid="ignore"):
        zs = coef / coef_sd
        sel = np.abs(zs) >= z
    pred = []
    for j in range(coef.shape[1]):
        idx = np.flatnonzero(sel[:, j])
        pred.append(idx[np.argsort(-np.abs(zs[idx, j]), kind="stable")])
    return {"z": zs, "selected": sel, "predictors": pred}
