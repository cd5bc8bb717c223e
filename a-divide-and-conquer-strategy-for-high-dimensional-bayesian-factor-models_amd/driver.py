"""Host twin of the reference driver and public entry point.

``divideconquer(Y, g, k, BURNIN, MCMC, thin, rho)`` mirrors the reference
function ``Sigmaout = divideconquer(Y,g,k,BURNIN,MCMC,thin,rho)``
(divideconquer.m:1): same arguments, same meaning, same output (the p x p
posterior-mean covariance in the permuted, standardised coordinates of
dc:186-195, quirk Q7).  The driver half (dc:29-87: zero-column removal,
P = p/g and K = k/g integrality, partition by randperm, standardisation,
hyper-parameters, initial draws) runs here on the host, as it does in MATLAB;
the hot loop (dc:90-197) runs on the GPU through the C ABI.

Differences a user should know:
  * The reference seeds nothing (no ``rng`` call); here ``seed`` selects both
    the host init draws (NumPy PCG64) and the on-device Philox stream.
  * ``init_draws`` / ``iter_draws`` inject standard variates (SURVEY
    Appendix B layout) instead — this is how the parity tests drive it.
  * ``return_info=True`` additionally returns varind (the permutation, which
    the reference never returns) and the kept-column index.
"""
from __future__ import annotations

import time

import numpy as np

from .diagnostics import waic as _waic, conditional_log_density as _cond_ld
from .sampler import Hyper, Sampler, count_nonzero_columns


def _require_two_rows(n):
    """dc:57: with n = 1 MATLAB's mean / var of the 1 x P x g array reduce along P, not along the rows, and the
    1/(n - 1) variance of the column-wise restatement (and of k_colstats) divides by zero."""
    if n < 2:
        raise ValueError(f"n = {n}: at least 2 rows are needed (dc:57 mean/var reduce along P when n = 1)")


def preprocess(Y, g, k):
    """dc:29-41. Returns (Y_kept, n, p, P, K, keep)."""
    Y = np.asarray(Y, dtype=np.float64)
    if Y.ndim != 2:
        raise ValueError("Y must be n x p (rows are observations, dc:30)")
    n, p = Y.shape
    _require_two_rows(n)
    keep = np.flatnonzero(np.count_nonzero(Y, axis=0) != 0)     # dc:31-38
    Y = Y[:, keep]
    p = keep.size                                                # dc:39
    if g < 1 or p % g or k % g:
        raise ValueError(f"P = p/g = {p}/{g} and K = k/g = {k}/{g} must be integers (dc:41)")
    return Y, n, p, p // g, k // g, keep


def preprocess_device(Y, g, k, device=0):
    """dc:29-41 with the column scan on the GPU (dcfm_count_nonzero_columns): returns
    (n, p, P, K, keep) — the kept width and index; the data itself is not copied, since
    dcfm_set_data_raw gathers the kept columns on the device through ``shard_columns``."""
    Y = np.asarray(Y, dtype=np.float64)
    if Y.ndim != 2:
        raise ValueError("Y must be n x p (rows are observations, dc:30)")
    n = Y.shape[0]
    _require_two_rows(n)
    keep = np.flatnonzero(count_nonzero_columns(Y, device=device) != 0)    # dc:31-38
    p = keep.size                                                          # dc:39
    if g < 1 or p % g or k % g:
        raise ValueError(f"P = p/g = {p}/{g} and K = k/g = {k}/{g} must be integers (dc:41)")
    return n, p, p // g, k // g, keep


def shard_columns(keep, varind, P, s0, gl):
    """Input column of every (local shard, position) of shards [s0, s0+gl): dc:50-54's
    Y(:, varind((m-1)*P+1 : m*P)) after the zero-column removal (dc:36), 0-based, shard-major
    — the ``cols`` argument of dcfm_set_data_raw."""
    return np.asarray(keep, dtype=np.int64)[np.asarray(varind)[s0 * P:(s0 + gl) * P]]


def partition_standardize(Y, g, varind):
    """dc:48-59: Yd(:,:,m) = Y(:,varind(block m)); centre; scale by 1./sqrt(var)."""
    n, p = Y.shape
    P = p // g
    Yd = np.empty((n, P, g))
    for m in range(g):
        Yd[:, :, m] = Y[:, varind[m * P:(m + 1) * P]]
    Md = Yd.mean(axis=0, keepdims=True)
    VYd = Yd.var(axis=0, ddof=1, keepdims=True)
    if np.any(VYd == 0):
        raise ValueError("a constant non-zero column has zero variance (dc:59 would divide by zero, Q13)")
    return (Yd - Md) * (1.0 / np.sqrt(VYd))


def preprocess_missing(Y, g, k):
    """dc:29-41 for data with holes (``divideconquer(..., impute=True)``): NaN marks a missing entry and the
    zero-column scan ignores it, so a column whose observed entries are all zero (or that has none) is dropped.
    Returns (Y_kept, n, p, P, K, keep) as ``preprocess``; Y_kept keeps its NaNs."""
    Y = np.asarray(Y, dtype=np.float64)
    if Y.ndim != 2:
        raise ValueError("Y must be n x p (rows are observations, dc:30)")
    n = Y.shape[0]
    keep = np.flatnonzero(np.count_nonzero(np.where(np.isnan(Y), 0.0, Y), axis=0) != 0)
    p = keep.size
    if g < 1 or p % g or k % g:
        raise ValueError(f"P = p/g = {p}/{g} and K = k/g = {k}/{g} must be integers (dc:41)")
    return Y[:, keep], n, p, p // g, k // g, keep


def partition_standardize_missing(Y, g, varind):
    """dc:48-59 on the observed entries: the partition of ``partition_standardize``, every column centred with the
    mean and scaled with the sample standard deviation (ddof = 1) of its observed entries.  Returns ``(Yd, mask)``,
    both n x P x g: the missing entries of Yd are 0 (the standardised column mean) and mask marks them.  A column
    with fewer than two observed entries or zero observed variance raises ValueError."""
    n, p = Y.shape
    P = p // g
    Yd = np.empty((n, P, g))
    for m in range(g):
        Yd[:, :, m] = Y[:, varind[m * P:(m + 1) * P]]
    mask = np.isnan(Yd)
    nobs = n - mask.sum(axis=0, keepdims=True)
    if np.any(nobs < 2):
        raise ValueError("a column has fewer than two observed entries: its variance (dc:57) is undefined")
    tot = np.where(mask, 0.0, Yd).sum(axis=0, keepdims=True)
    Md = tot / nobs
    dev = np.where(mask, 0.0, Yd - Md)
    VYd = (dev * dev).sum(axis=0, keepdims=True) / (nobs - 1)
    if np.any(VYd == 0):
        raise ValueError("a column's observed entries are constant: zero variance (dc:59 would divide by zero, Q13)")
    return dev * (1.0 / np.sqrt(VYd)), mask


def observed_moments(Y):
    """``column_moments`` on the observed (non-NaN) entries: (mean, sd) of every input column, ddof = 1; a column
    with fewer than two observed entries gets sd 0, one with none mean 0."""
    Y = np.asarray(Y, dtype=np.float64)
    mask = np.isnan(Y)
    nobs = Y.shape[0] - mask.sum(axis=0)
    mean = np.where(mask, 0.0, Y).sum(axis=0) / np.maximum(nobs, 1)
    dev = np.where(mask, 0.0, Y - mean)
    return mean, np.sqrt((dev * dev).sum(axis=0) / np.maximum(nobs - 1, 1)) * (nobs > 1)


def unstandardize_imputation(imp, Y, mean, sd, keep, varind, s0=0) -> dict:
    """``Sampler.imputed()`` of the shards [s0, s0 + g_local) in the data's units and the input's column order:
    ``mean`` (n, p_orig) is Y with its NaNs replaced by mean_col + sd_col * (posterior mean), ``sd`` (n, p_orig) the
    total predictive standard deviation times sd_col, 0 at observed entries.  Missing entries of dropped all-zero
    columns come back 0 with sd 0; those of other ranks' shards stay NaN."""
    Y = np.asarray(Y, dtype=np.float64)
    mean, sd = np.asarray(mean, dtype=np.float64), np.asarray(sd, dtype=np.float64)
    n, P, gl = imp["mean"].shape
    cols = output_columns(keep, varind)[s0 * P:(s0 + gl) * P]
    out_mean, out_sd = Y.copy(), np.zeros(Y.shape)
    dropped = np.setdiff1d(np.arange(Y.shape[1]), np.asarray(keep))
    out_mean[:, dropped] = np.where(np.isnan(Y[:, dropped]), 0.0, Y[:, dropped])
    mk = imp["mask"].reshape(n, P * gl, order="F")
    mu = mean[cols] + sd[cols] * imp["mean"].reshape(n, P * gl, order="F")
    out_mean[:, cols] = np.where(mk, mu, Y[:, cols])
    out_sd[:, cols] = np.where(mk, sd[cols] * imp["sd_total"].reshape(n, P * gl, order="F"), 0.0)
    return {"mean": out_mean, "sd": out_sd, "count": imp["count"]}


class _HostInitDraws:
    """Standard variates for dc:50-83 from NumPy (the reference uses MATLAB's stream)."""

    def __init__(self, seed, n, p, g, K, hyper: Hyper):
        r = np.random.Generator(np.random.PCG64(np.random.SeedSequence([int(seed), 0, 0])))
        P = p // g
        self.varind = r.permutation(p)
        self.ps0 = r.standard_gamma(hyper.as_, size=(P, 1, g))
        self.X0 = r.standard_normal((n, K))
        self.psi0 = r.standard_gamma(hyper.df / 2.0, size=(P, K, g))
        self.Z0 = np.empty((n, K, g))
        self.delta0 = np.empty((K, g))
        for m in range(g):
            self.Z0[:, :, m] = r.standard_normal((n, K))
            self.delta0[0, m] = r.standard_gamma(hyper.ad1)
            if K > 1:
                self.delta0[1:, m] = r.standard_gamma(hyper.ad2, size=K - 1)


class _HostVarind:
    """dc:50 varind = randperm(p) alone (the first draw of _HostInitDraws' stream)."""

    def __init__(self, seed, p):
        r = np.random.Generator(np.random.PCG64(np.random.SeedSequence([int(seed), 0, 0])))
        self.varind = r.permutation(p)


def initial_state(n, P, K, g, rho, hyper: Hyper, init) -> dict:
    """dc:68-87 from standard variates ``init`` (fields varind, ps0, X0, psi0, Z0, delta0)."""
    ps = (1.0 / hyper.bs) * np.asarray(init.ps0)                 # dc:69
    X = np.array(init.X0, dtype=float)                           # dc:71
    psi = (2.0 / hyper.df) * np.asarray(init.psi0)               # dc:73
    Z = np.array(init.Z0, dtype=float)                           # dc:80
    delta = np.empty((K, 1, g))
    delta[0, 0, :] = hyper.bd1 * init.delta0[0, :]               # dc:83
    delta[1:, 0, :] = hyper.bd2 * init.delta0[1:, :]
    tauh = np.cumprod(delta, axis=0)                             # dc:85 (per shard)
    Plam = psi * np.transpose(tauh, (1, 0, 2))                   # dc:86
    eta = np.sqrt(rho) * X[:, :, None] + np.sqrt(1 - rho) * Z   # dc:81
    return {
        "Lambda": np.zeros((P, K, g)), "ps": ps, "omega": ps[:, 0, :].copy(),   # dc:70,84 (Q1)
        "psi": psi, "Plam": Plam, "X": X, "Z": Z, "eta": eta, "delta": delta, "tauh": tauh,
    }


def local_state(state: dict, s0: int, gl: int) -> dict:
    """Slice the per-shard fields to shards [s0, s0+gl); X, delta, tauh stay whole."""
    out = {}
    for f, a in state.items():
        if f in ("X", "delta", "tauh"):
            out[f] = a
        else:
            out[f] = a[..., s0:s0 + gl]
    return out


def divideconquer(Y, g, k, BURNIN, MCMC, thin, rho, *, seed=0, hyper: Hyper = Hyper(),
                  init_draws=None, iter_draws=None, nranks=1, rank=0, device=0, comm_uid=None,
                  asm_batch=0, return_info=False, device_ingest=True, device_init=True, return_sd=False,
                  n_components=0, rhs=None, probes=None, precision_probes=None, return_precision=False, loglik=False,
                  predict=None, impute=False, return_partial=False, return_corr=False, regress=None):
    """Sigmaout = divideconquer(Y,g,k,BURNIN,MCMC,thin,rho)   (divideconquer.m:1).

    ``device_ingest`` (default): the zero-column scan and the partition/standardisation
    (dc:31-59) run on the GPU (dcfm_count_nonzero_columns, dcfm_set_data_raw); False
    keeps them on the host (NumPy) and uploads Yd.  ``device_init`` (default, unless
    ``init_draws`` are injected): the initial state of dc:68-87 is drawn on the GPU from
    the Philox stream (dcfm_init_state); only varind (dc:50) is drawn on the host.

    Multi-GPU: call on every rank with the same arguments plus nranks/rank/device
    and the 128-byte RCCL id (``Sampler.unique_id()`` on rank 0, broadcast by
    the caller).  Every rank returns the full Sigmaout.

    ``return_sd``: also accumulate the second moment of the per-sample covariance on the device
    (DCFM_FLAG_SIGMA_M2) and return ``(Sigmaout, Sigmasd)`` — or ``(Sigmaout, Sigmasd, info)`` with
    ``return_info`` — where Sigmasd is the p x p posterior standard deviation of every entry over
    the saved samples, in Sigmaout's coordinates.

    ``return_precision``: also accumulate the posterior mean of the precision matrix on the device
    (DCFM_FLAG_PRECISION_MEAN) and append Theta = (1/effsamp) sum_s inv(Sigma(s)) -- p x p, in Sigmaout's
    coordinates; E[inv(Sigma)], not the inverse of Sigmaout -- to the returned tuple after Sigmasd (if
    requested) and before the ``n_components`` dict.  ``unpermute_precision`` takes it back to the input's
    column order and ``diagnostics.partial_correlations`` reads the partial correlations off it.

    ``return_partial``: also accumulate the posterior mean and second moment of the per-sample partial
    correlations on the device (DCFM_FLAG_PARTIAL_CORR) and append ``{"mean", "sd"}`` after Theta (if requested)
    and before the ``n_components`` dict: the posterior mean (with Sigmaout's 1/effsamp scaling, quirk Q8: its diagonal is
    saved/effsamp, 1 when thin divides MCMC and BURNIN) and the posterior standard deviation of every partial correlation, p_orig x p_orig in the *input's* column order
    (``unpermute_partial``: partial correlations do not change with the columns' scaling, so this is a pure
    un-permutation; dropped all-zero columns get NaN, with 1 (mean) and 0 (sd) on the diagonal).
    ``diagnostics.partial_correlation_edges`` turns the pair into the edges of the graphical model.

    ``return_corr``: also accumulate the posterior mean and second moment of the per-sample correlation matrix
    ``Sigma(s) / sqrt(v v')``, ``v = diag(Sigma(s))``, and of the communalities ``h_a(s) = |Lambda_a(s)|^2 / v_a(s)``
    on the device (DCFM_FLAG_CORR) and append ``{"mean", "sd", "communality", "communality_sd"}`` after the
    ``return_partial`` dict (if requested) and before the ``n_components`` dict: the posterior mean (1/effsamp
    scaling, quirk Q8) and standard deviation of every correlation, p_orig x p_orig, and of every variable's
    communality, p_orig entries, in the *input's* column order (``unpermute_corr`` / ``unpermute_communality``:
    correlations and communalities do not change with the columns' scaling, so these are pure un-permutations;
    dropped all-zero columns get NaN, with 1 (mean) and 0 (sd) on the matrices' diagonal).  The mean is the
    posterior mean of the correlation, not the plug-in ``diagnostics.correlation(Sigmaout)``.

    ``n_components`` > 0: also the leading principal components of Sigmaout, found on the device
    (Sampler.sigma_eigs: ``values``, ``vectors`` p x n_components, ``resid``, ``passes``,
    ``converged``), appended to the returned tuple after Sigmasd (if requested) and before info.  The
    vectors are in Sigmaout's coordinates; ``unpermute_vectors`` takes them back to the input's.
    With several ranks every rank takes part and returns the same dict.

    ``rhs``: right-hand sides B, (p_orig,) or (p_orig, nv) with one row per column of Y in the input's
    column order.  B is taken into Sigmaout's coordinates (``permute_vectors`` without sd: the rows of
    dropped all-zero columns fall away) and Sigmaout x = B is solved on the device
    (Sampler.sigma_solve with its defaults: tol 1e-10, at most min(2 p, 1000) steps); a dict ``{"x", "relres", "iters",
    "quad"}``, x in Sigmaout's coordinates, is appended to the returned tuple after the
    ``n_components`` dict (if requested) and before info.  Sigmaout is the standardised covariance S;
    the unstandardised one is D S D with D = diag(sd) (the sample standard deviations of the kept
    columns in Sigmaout's order), so its precision applied to b is D^-1 S^-1 D^-1 b:
    ``x = sigma_solve(permute_vectors(b, keep, varind, sd=sd))``, then
    ``unpermute_vectors(x / sd[:, None], keep, varind, p_orig)``.

    ``probes``: probe vectors V, (p_orig,) or (p_orig, nv) with nv <= 32 and one row per column of Y in
    the input's column order.  V is taken into Sigmaout's coordinates (``permute_vectors`` without sd:
    the rows of dropped all-zero columns fall away) and ``V' Sigma(s) V`` is recorded on the device for
    every saved sample s (Sampler.set_probes with its default capacity, mcmc // thin); a dict
    ``{"draws", "mean", "sd"}`` -- draws (S, nv, nv), their mean and their standard deviation over the
    draws (population form, as Sigmasd) -- is appended to the returned tuple after the ``rhs`` dict (if
    requested) and before info.  ``diagnostics.summarize_probes`` gives quantiles and the per-draw
    correlations.  For the unstandardised covariance D S D probe with D v:
    ``Sampler.set_probes(permute_vectors(v, keep, varind) * sd[:, None])``, sd the sample standard
    deviations of the kept columns in Sigmaout's order.

    ``precision_probes``: probe vectors V as for ``probes`` (nv = 0, a (p_orig, 0) block, is allowed),
    permuted exactly as ``probes`` is; ``V' Sigma(s)^-1 V`` and ``log det Sigma(s)`` are recorded on the
    device for every saved sample s (Sampler.set_precision_probes, capacity mcmc // thin) and a dict
    ``{"draws", "logdet", "mean", "sd"}`` -- draws (S, nv, nv), logdet (S,), mean and sd of the draws -- is
    appended after the ``probes`` dict (if requested) and before info.  Held-out log density: a new row
    y in the input's column order becomes the probe
    ``permute_vectors(((y - mean) / sd)[:, None], keep, varind)`` (mean and sd the training columns'
    sample mean and standard deviation, in the input's order), and
    ``diagnostics.heldout_log_density(draws, logdet, p)`` gives the per-sample densities and their
    log-mean-exp (lppd) in the standardised units; a density in the original units subtracts
    ``sum(log sd)`` over the kept columns.

    ``loglik``: the pointwise log-likelihood of the training rows needs no held-out data: with True,
    ``ll[s, i] = log N(y_i; 0, Sigma(s))`` of every row i of the standardised data under every saved sample s
    is recorded on the device (Sampler.set_loglik, capacity mcmc // thin) and a dict ``{"ll", "logdet",
    "waic"}`` -- ll (S, n), logdet (S,) and ``diagnostics.waic(ll)`` (lppd, p_waic, elpd_waic, waic, se and the
    per-point terms) -- is appended after the ``precision_probes`` dict (if requested) and before info.
    Standardised units, as above; runs that are compared over g, k or rho must use the same Y.

    ``predict``: ``(Ynew, observed)`` -- new rows Ynew, (nt, p_orig) or (p_orig,) with nt <= 32, in the data's
    units and the input's column order, and a boolean mask ``observed`` (p_orig,), one for all rows: which
    variables of the new rows are known.  The rows are centred and scaled with the training columns' mean
    and standard deviation (dc:57-59; ``standardize_rows``), taken into Sigmaout's coordinates, and the
    Gaussian conditional of the other variables given the observed ones is accumulated on the device over the
    saved samples (Sampler.set_predict, capacity mcmc // thin; one rank only).  A dict ``{"mean",
    "sd_between", "sd_total", "log_density", "lppd", "count"}`` is appended after the ``loglik`` dict (if
    requested) and before info: mean (nt, p_orig) the posterior conditional mean in the data's units and the
    input's column order, sd_between and sd_total (nt, p_orig) the between-sample and the total predictive
    standard deviation (``unstandardize_prediction``), log_density (S, nt) the log density of each row's
    observed part per saved sample and lppd (nt,) their log-mean-exp (``diagnostics.conditional_log_density``;
    standardised units).  Entries of Ynew at unobserved positions are ignored.  A dropped all-zero column
    counts as unobserved and gets mean 0 and sd 0.

    ``impute``: with True the NaN entries of Y are missing training data (without it a NaN is handled exactly as
    before: it runs through the sweep and ends the chain in DCFM_ERR_NUMERIC).  dc:31-59 then run on the host
    whatever ``device_ingest`` says: the zero-column scan ignores NaN (``preprocess_missing``), every column is
    centred and scaled with the mean and sample standard deviation of its observed entries
    (``partition_standardize_missing``; a kept column with fewer than two observed entries or zero observed
    variance raises ValueError), and the missing entries are uploaded as 0 together with their mask
    (Sampler.set_missing, capacity mcmc // thin): every iteration then redraws them on the device from their
    conditional given eta, Lambda and ps.  A dict ``{"mean", "sd", "count"}`` is appended after the ``predict``
    dict (if requested) and before info: mean (n, p_orig) is the input with its NaNs replaced by the posterior
    mean in the data's units, sd (n, p_orig) the total predictive standard deviation in the data's units, 0 at
    observed entries (``unstandardize_imputation``).  Missing entries of dropped all-zero columns come back 0
    with sd 0; with several ranks every rank fills in the entries of its own shards.  With ``predict`` the
    training moments used for the new rows are the observed-entry ones.  Not together with ``loglik``
    (ValueError): that would be the likelihood of the completed data.

    ``regress``: up to 32 distinct column indices of Y (0-based, the input's column order): the responses of a
    Bayesian factor regression on all the other columns.  They are taken into Sigmaout's coordinates (a response
    that is a dropped all-zero column raises ValueError) and the posterior moments of the per-sample coefficients
    ``Sigma_OO(s)^-1 Sigma_OR(s)``, of the residual covariance and of R^2 are accumulated on the device
    (DCFM_FLAG_REGRESSION, Sampler.set_regression).  A dict ``{"coef", "coef_sd", "intercept", "resid_cov",
    "resid_cov_sd", "r2", "r2_sd", "count", "responses"}`` is appended after the ``impute`` dict (if requested) and
    before info, in the data's units and the input's column order (``unstandardize_regression``): coef and coef_sd
    (p_orig, q), ``y[:, responses[j]] ~ intercept[j] + y @ coef[:, j]``, with 0 in the rows of the responses and of
    the dropped columns.
    """
    t0 = time.perf_counter()                                     # dc:29 tic
    if impute and loglik:
        raise ValueError("impute=True with loglik=True: the rows' log-likelihood would be that of the completed "
                         "data, not of the observed entries")
    if impute:
        device_ingest = False
        Yk, n, p, P, K, keep = preprocess_missing(Y, g, k)
    elif device_ingest:
        Y = np.asarray(Y, dtype=np.float64)
        n, p, P, K, keep = preprocess_device(Y, g, k, device=device)
    else:
        Yk, n, p, P, K, keep = preprocess(Y, g, k)
    N = BURNIN + MCMC                                            # dc:45
    on_device_init = device_init and init_draws is None
    if init_draws is not None:
        init = init_draws
    elif on_device_init:                                         # dc:50 only; dc:68-87 on the GPU
        init = _HostVarind(seed, p)
    else:
        init = _HostInitDraws(seed, n, p, g, K, hyper)
    if impute:
        Yd, miss = partition_standardize_missing(Yk, g, np.asarray(init.varind))
    elif not device_ingest:
        Yd = partition_standardize(Yk, g, np.asarray(init.varind))
    state = None if on_device_init else initial_state(n, P, K, g, rho, hyper, init)
    resp = None
    if regress is not None:                                      # the responses in Sigmaout's coordinates
        rc = np.asarray(regress, dtype=np.int64).reshape(-1)
        where = {int(c): a for a, c in enumerate(output_columns(keep, init.varind))}
        gone = [int(c) for c in rc if int(c) not in where]
        if gone:
            raise ValueError(f"regress: columns {gone} of Y are all zero (dropped, dc:36-39) or out of range")
        resp = np.array([where[int(c)] for c in rc], dtype=np.int64)
    gl = g // nranks
    s0 = rank * gl
    smp = Sampler(n, P, g, K, rho, BURNIN, MCMC, thin, hyper=hyper, seed=seed, nranks=nranks,
                  rank=rank, device=device, inject_draws=iter_draws is not None, asm_batch=asm_batch,
                  sigma_m2=return_sd, precision_mean=return_precision, partial_corr=return_partial,
                  corr=return_corr, regression=resp is not None)
    try:
        if nranks > 1:
            if comm_uid is None:
                raise ValueError("nranks > 1 needs comm_uid (Sampler.unique_id() from rank 0)")
            smp.comm_init(comm_uid)
        if device_ingest:                                        # dc:48-59 on the device
            smp.set_data_raw(Y, shard_columns(keep, init.varind, P, s0, gl))
        else:
            smp.set_data(Yd[:, :, s0:s0 + gl])
        if impute:
            smp.set_missing(miss[:, :, s0:s0 + gl])
        if state is None:
            smp.init_state()
        else:
            smp.set_state(local_state(state, s0, gl))
        if iter_draws is not None:
            smp.set_draws(iter_draws, 1, N)
        if probes is not None:
            smp.set_probes(permute_vectors(probes, keep, init.varind))
        if precision_probes is not None:
            smp.set_precision_probes(permute_vectors(precision_probes, keep, init.varind))
        if loglik:
            smp.set_loglik()
        if predict is not None:
            Yraw = np.asarray(Y, dtype=np.float64)
            cmean, csd = observed_moments(Yraw) if impute else column_moments(Yraw)
            Ystd, obs_in = standardize_rows(predict[0], predict[1], cmean, csd, keep, init.varind)
            smp.set_predict(Ystd, obs_in)
        if resp is not None:
            smp.set_regression(resp)
        smp.run(1, N)                                            # dc:90-197
        Sigmaout = smp.get_sigma()
        Sigmasd = smp.get_sigma_moment("sd") if return_sd else None
        Theta = smp.get_precision_mean() if return_precision else None
        pcr = None
        if return_partial:
            Rm, Rs = smp.get_partial_corr("mean"), smp.get_partial_corr("sd")
            if Rm is not None:                                   # rank 0
                pcr = {"mean": unpermute_partial(Rm, keep, init.varind, np.asarray(Y).shape[1]),
                       "sd": unpermute_partial(Rs, keep, init.varind, np.asarray(Y).shape[1], diag=0.0)}
        crr = None
        if return_corr:
            Cm, Cs = smp.get_corr("mean"), smp.get_corr("sd")
            if Cm is not None:                                   # rank 0
                p0 = np.asarray(Y).shape[1]
                crr = {"mean": unpermute_corr(Cm, keep, init.varind, p0),
                       "sd": unpermute_corr(Cs, keep, init.varind, p0, diag=0.0),
                       "communality": unpermute_communality(smp.get_communality("mean"), keep, init.varind, p0),
                       "communality_sd": unpermute_communality(smp.get_communality("sd"), keep, init.varind, p0)}
        pcs = smp.sigma_eigs(int(n_components)) if n_components > 0 else None
        sol = None
        if rhs is not None:
            x, si = smp.sigma_solve(permute_vectors(rhs, keep, init.varind), return_info=True)
            sol = {"x": x, "relres": si["relres"], "iters": si["iters"], "quad": si["quad"]}
        prb = None
        if probes is not None:
            q = smp.probe_draws()
            prb = {"draws": q, "mean": q.mean(axis=0), "sd": q.std(axis=0)}
        prc = None
        if precision_probes is not None:
            q, ld = smp.precision_draws()
            prc = {"draws": q, "logdet": ld, "mean": q.mean(axis=0), "sd": q.std(axis=0)}
        llk = None
        if loglik:
            ll, _, ld = smp.loglik_draws(parts=True)
            llk = {"ll": ll, "logdet": ld, "waic": _waic(ll) if ll.shape[0] >= 2 else None}   # waic needs two samples
        prd = None
        if predict is not None:
            pr = smp.predict()
            prd = unstandardize_prediction(pr, cmean, csd, keep, init.varind, Yraw.shape[1])
            cl = _cond_ld(pr["maha"], pr["logdet"], int(obs_in.sum())) if pr["count"] else None
            prd["log_density"] = cl["per_sample"] if cl else np.zeros((0, Ystd.shape[1]))
            prd["lppd"] = cl["lppd"] if cl else np.full(Ystd.shape[1], np.nan)
            prd["count"] = pr["count"]
        imp = None
        if impute:
            Yraw = np.asarray(Y, dtype=np.float64)
            omean, osd = observed_moments(Yraw)
            imp = unstandardize_imputation(smp.imputed(), Yraw, omean, osd, keep, init.varind, s0)
        reg = None
        if resp is not None:
            Yraw = np.asarray(Y, dtype=np.float64)
            rmean, rsd = observed_moments(Yraw) if impute else column_moments(Yraw)
            reg = unstandardize_regression(smp.regression(), rmean, rsd, keep, init.varind, Yraw.shape[1])
    finally:
        smp.close()
    elapsed = time.perf_counter() - t0                           # dc:200 toc
    out = (Sigmaout, Sigmasd) if return_sd else (Sigmaout,)
    if return_precision:
        out += (Theta,)
    if return_partial:
        out += (pcr,)
    if return_corr:
        out += (crr,)
    if n_components > 0:
        out += (pcs,)
    if rhs is not None:
        out += (sol,)
    if probes is not None:
        out += (prb,)
    if precision_probes is not None:
        out += (prc,)
    if loglik:
        out += (llk,)
    if predict is not None:
        out += (prd,)
    if impute:
        out += (imp,)
    if regress is not None:
        out += (reg,)
    if return_info:
        out += ({"varind": np.asarray(init.varind), "keep": keep, "n": n, "p": p, "P": P,
                 "K": K, "N": N, "seconds": elapsed},)
    return out if len(out) > 1 else out[0]


def column_moments(Y):
    """(mean, sd) of every input column of the training data Y (n x p_orig): the sample mean and the sample
    standard deviation (ddof = 1) that dc:57-59 centres and scales with; an all-zero column has sd 0."""
    Y = np.asarray(Y, dtype=np.float64)
    return Y.mean(axis=0), Y.std(axis=0, ddof=1)


def standardize_rows(Ynew, observed, mean, sd, keep, varind):
    """New rows in the data's units into the coordinates the sweep works in.  Ynew is (nt, p_orig) or (p_orig,)
    in the input's column order, observed a boolean (p_orig,) mask, mean and sd the training columns' moments
    (``column_moments``).  Returns ``(Ystd, obs)``: Ystd (p, nt) = (Ynew - mean) / sd on the kept columns in
    Sigmaout's order (``permute_vectors``), new rows as columns, zero at the unobserved positions (whatever
    Ynew holds there, NaN included), and obs (p,) uint8.  Dropped all-zero columns fall away: they count as
    unobserved."""
    Yn = np.asarray(Ynew, dtype=np.float64)
    Yn = Yn[None, :] if Yn.ndim == 1 else Yn
    mean, sd = np.asarray(mean, dtype=np.float64), np.asarray(sd, dtype=np.float64)
    ob = np.asarray(observed).astype(bool).reshape(-1)
    if Yn.ndim != 2 or Yn.shape[1] != mean.size or ob.size != mean.size:
        raise ValueError(f"Ynew must be (nt, {mean.size}) or ({mean.size},) and observed ({mean.size},), "
                         f"got {Yn.shape} and {ob.shape}")
    obs = permute_vectors(ob.astype(np.float64), keep, varind) != 0
    cols = output_columns(keep, varind)
    Ystd = np.zeros((cols.size, Yn.shape[0]))
    Ystd[obs] = ((Yn[:, cols[obs]] - mean[cols[obs]]) / sd[cols[obs]]).T
    return Ystd, obs.astype(np.uint8)


def unstandardize_prediction(pred, mean, sd, keep, varind, p_orig) -> dict:
    """``Sampler.predict()``'s mean, sd_between and sd_total ((p, nt), standardised, Sigmaout's order) in the
    data's units and the input's column order, new rows as rows: mean (nt, p_orig) = mean_col + sd_col * yhat,
    the standard deviations times sd_col.  Dropped all-zero columns get mean 0 and sd 0."""
    mean, sd = np.asarray(mean, dtype=np.float64), np.asarray(sd, dtype=np.float64)
    cols = output_columns(keep, varind)
    out = {}
    for f in ("mean", "sd_between", "sd_total"):
        v = np.asarray(pred[f], dtype=np.float64) * sd[cols][:, None]
        if f == "mean":
            v = v + mean[cols][:, None]
        out[f] = unpermute_vectors(v, keep, varind, p_orig).T.copy()
    return out


def unstandardize_regression(reg, mean, sd, keep, varind, p_orig, fill=0.0) -> dict:
    """``Sampler.regression()``'s dict (standardised, Sigmaout's order) in the data's units and the input's column
    order.  With sd_a the training columns' standard deviations and r_j the responses, a standardised coefficient
    b_aj (y_rj / sd_rj ~ sum_a b_aj y_a / sd_a) becomes ``coef[a, j] = b_aj sd_rj / sd_a`` and its SD scales the
    same way; ``intercept[j] = mean_rj - sum_a coef[a, j] mean_a``; resid_cov and its SD are scaled by sd_R on both
    sides; R^2 does not change with the columns' scaling.  coef and coef_sd are (p_orig, q); dropped all-zero
    columns get ``fill``.  ``responses`` are the responses' columns of Y."""
    mean, sd = np.asarray(mean, dtype=np.float64), np.asarray(sd, dtype=np.float64)
    cols = output_columns(keep, varind)
    r = np.asarray(reg["responses"], dtype=np.int64)
    sdk, sdr = sd[cols], sd[cols[r]]
    scale = sdr[None, :] / sdk[:, None]
    coef = np.asarray(reg["coef"], dtype=np.float64) * scale
    out = {"coef": unpermute_vectors(coef, keep, varind, p_orig, fill=fill),
           "coef_sd": unpermute_vectors(np.asarray(reg["coef_sd"], dtype=np.float64) * scale, keep, varind, p_orig,
                                        fill=fill),
           "intercept": mean[cols[r]] - mean[cols] @ coef,
           "resid_cov": np.asarray(reg["resid_cov"], dtype=np.float64) * np.outer(sdr, sdr),
           "resid_cov_sd": np.asarray(reg["resid_cov_sd"], dtype=np.float64) * np.outer(sdr, sdr),
           "r2": np.asarray(reg["r2"], dtype=np.float64).copy(),
           "r2_sd": np.asarray(reg["r2_sd"], dtype=np.float64).copy(),
           "count": reg["count"], "responses": cols[r].copy()}
    return out


def truth_factors(Lam0, sig2, Y, keep, varind):
    """Truth Sigma0 = Lam0 Lam0' + diag(sig2) as (U, s) in Sigmaout's coordinates: kept
    columns (dc:36-39), permuted by varind (dc:50-54), standardised by the sample
    standard deviations (dc:57-59), so Sigma0_out = U U' + diag(s) — the low-rank form
    dcfm_sigma_error takes."""
    Y = np.asarray(Y, dtype=np.float64)
    cols = np.asarray(keep)[np.asarray(varind)]
    sd = Y[:, cols].std(axis=0, ddof=1)
    U = np.asarray(Lam0, dtype=np.float64)[cols] / sd[:, None]
    s = np.asarray(sig2, dtype=np.float64)[cols] / (sd * sd)
    return U, s


def output_columns(keep, varind):
    """Input column index of each Sigmaout row/column: kept columns (dc:36-39) in the
    varind order of the partition (dc:50-54) — Sigmaout's coordinates (quirk Q7)."""
    return np.asarray(keep)[np.asarray(varind)]


def unpermute_sigma(S, keep, varind, p_orig, sd=None, fill=0.0):
    """Sigmaout back in the input's column order: S[a, b] goes to (cols[a], cols[b]) with
    cols = output_columns(keep, varind); rows/columns of dropped (all-zero, dc:36-39)
    columns get ``fill``.  With ``sd`` (the sample standard deviations of the kept
    columns in Sigmaout's order, dc:57) the standardisation is undone: S_ab sd_a sd_b.
    The reference returns the permuted, standardised matrix and leaves this to the
    caller.  The posterior standard deviation Sigmasd of
    ``divideconquer(..., return_sd=True)`` goes through the same call: a standard deviation
    scales like the entry itself, sd(S_ab sd_a sd_b) = sd(S_ab) sd_a sd_b."""
    S = np.asarray(S, dtype=np.float64)
    cols = output_columns(keep, varind)
    if sd is not None:
        sd = np.asarray(sd, dtype=np.float64)
        S = S * sd[:, None] * sd[None, :]
    out = np.full((p_orig, p_orig), fill, dtype=np.float64)
    out[np.ix_(cols, cols)] = S
    return out


def unpermute_precision(T, keep, varind, p_orig, sd=None, fill=0.0):
    """The precision mean Theta of ``divideconquer(..., return_precision=True)`` back in the input's column
    order: T[a, b] goes to (cols[a], cols[b]) with cols = output_columns(keep, varind); rows/columns of
    dropped (all-zero, dc:36-39) columns get ``fill``.  With ``sd`` (the sample standard deviations of the
    kept columns in Sigmaout's order, dc:57) the standardisation is undone: the unstandardised covariance
    is D S D with D = diag(sd) and (D S D)^-1 = D^-1 S^-1 D^-1, so the entry is *divided*,
    T_ab / (sd_a sd_b) -- the inverse of what ``unpermute_sigma`` does, so that the two results stay
    inverse to each other on the kept block."""
    T = np.asarray(T, dtype=np.float64)
    cols = output_columns(keep, varind)
    if sd is not None:
        sd = np.asarray(sd, dtype=np.float64)
        T = T / sd[:, None] / sd[None, :]
    out = np.full((p_orig, p_orig), fill, dtype=np.float64)
    out[np.ix_(cols, cols)] = T
    return out


def unpermute_partial(R, keep, varind, p_orig, fill=np.nan, diag=1.0):
    """A partial-correlation matrix in Sigmaout's coordinates (``Sampler.get_partial_corr``, or
    ``diagnostics.partial_correlations`` of a precision matrix) back in the input's column order: R[a, b] goes
    to (cols[a], cols[b]) with cols = output_columns(keep, varind).  Partial correlations are invariant to
    the columns' scaling -- (D T D)_ab / sqrt((D T D)_aa (D T D)_bb) = T_ab / sqrt(T_aa T_bb) for a positive
    diagonal D -- so, unlike ``unpermute_sigma`` and ``unpermute_precision``, there is no ``sd``: a pure
    un-permutation.  Rows/columns of dropped (all-zero, dc:36-39) columns get ``fill`` (NaN: the model says
    nothing about them) with ``diag`` on their diagonal (1, a variable with itself; pass 0 for a matrix of
    standard deviations)."""
    out = unpermute_sigma(R, keep, varind, p_orig, fill=fill)
    dropped = np.setdiff1d(np.arange(p_orig), output_columns(keep, varind))
    out[dropped, dropped] = diag
    return out


def unpermute_corr(R, keep, varind, p_orig, fill=np.nan, diag=1.0):
    """A correlation matrix in Sigmaout's coordinates (``Sampler.get_corr``, or ``diagnostics.correlation`` of a
    covariance) back in the input's column order.  Correlations are invariant to the columns' scaling --
    (D S D)_ab / sqrt((D S D)_aa (D S D)_bb) = S_ab / sqrt(S_aa S_bb) for a positive diagonal D -- so this is
    ``unpermute_partial``'s pure un-permutation: dropped (all-zero, dc:36-39) columns get ``fill`` with ``diag``
    on their diagonal (1; pass 0 for a matrix of standard deviations)."""
    return unpermute_partial(R, keep, varind, p_orig, fill=fill, diag=diag)


def unpermute_communality(h, keep, varind, p_orig, fill=np.nan):
    """Per-variable values in Sigmaout's coordinates (``Sampler.get_communality``) back in the input's column
    order: entry a goes to cols[a] with cols = output_columns(keep, varind).  A communality is a ratio of two
    variances of the same column, so there is no ``sd``; dropped (all-zero, dc:36-39) columns get ``fill``
    (NaN: the model says nothing about them)."""
    h = np.asarray(h, dtype=np.float64)
    if h.ndim != 1:
        raise ValueError(f"h must be a vector of p entries, got {h.shape}")
    return unpermute_vectors(h, keep, varind, p_orig, fill=fill)


def unpermute_vectors(V, keep, varind, p_orig, sd=None, fill=0.0):
    """Vectors in Sigmaout's coordinates (rows of V: (p,) or (p, r), e.g. the ``vectors`` of
    ``Sampler.sigma_eigs``) back in the input's column order: row a goes to row cols[a] with
    cols = output_columns(keep, varind); rows of dropped (all-zero, dc:36-39) columns get
    ``fill`` -- the row analogue of ``unpermute_sigma``.  With ``sd`` (the sample standard
    deviations of the kept columns in Sigmaout's order) row a is scaled by sd_a: the vectors are
    then loadings in data units (directions of the unstandardised covariance's factor
    diag(sd) V) and are no longer orthonormal."""
    V = np.asarray(V, dtype=np.float64)
    cols = output_columns(keep, varind)
    if V.shape[0] != cols.size:
        raise ValueError(f"V must have p = {cols.size} rows, got {V.shape}")
    if sd is not None:
        sd = np.asarray(sd, dtype=np.float64).reshape(-1)
        V = V * (sd if V.ndim == 1 else sd[:, None])
    out = np.full((p_orig,) + V.shape[1:], fill, dtype=np.float64)
    out[cols] = V
    return out


def permute_vectors(B, keep, varind, sd=None):
    """Vectors in the input's column order (rows of B: (p_orig,) or (p_orig, nv), one per column of
    Y) into Sigmaout's coordinates: row a of the result is row cols[a] of B with
    cols = output_columns(keep, varind); the rows of dropped (all-zero, dc:36-39) columns fall away.
    The exact inverse of ``unpermute_vectors`` on the kept rows.  With ``sd`` (the sample standard
    deviations of the kept columns in Sigmaout's order) row a is divided by sd_a, which undoes
    ``unpermute_vectors(..., sd=sd)`` -- and is the D^-1 b of the unstandardised precision
    D^-1 S^-1 D^-1 b (``divideconquer(..., rhs=)``)."""
    B = np.asarray(B, dtype=np.float64)
    cols = output_columns(keep, varind)
    if B.ndim not in (1, 2) or B.shape[0] <= int(cols.max(initial=-1)):
        raise ValueError(f"B must have one row per input column (more than {int(cols.max(initial=-1))}), got {B.shape}")
    out = B[cols]
    if sd is not None:
        sd = np.asarray(sd, dtype=np.float64).reshape(-1)
        out = out / (sd if B.ndim == 1 else sd[:, None])
    return out
