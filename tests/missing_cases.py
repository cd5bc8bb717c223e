"""Shared setup of the missing-data tests (test_missing_host.py on the CPU, test_gpu_missing.py on the GPU):
the shapes, the mask patterns, the NumPy restatement of the imputation step (dcfm_set_missing, csrc/impute.hip)
and of its yy rule, and the host twin of the step's Philox normals.

The step, for every missing (i, j) of shard m:  mu = sum_k eta_ik lambda_jk,  Y_ij = mu + z_ij / sqrt(ps_j), z the
standard normal at the counter (site 13, shard m, row j, index i, iteration); then yy_j = (sum of squares of the
observed entries) + (sum of squares of the missing ones) for every column with a missing entry.
"""
import numpy as np

SITE_IMPUTE = 13
UNFUSED, EXACT_RESIDUAL, COMM_SELF, GUARD_ALL = 0x2, 0x10, 0x20, 0x40      # include/dcfm.h
CHAIN_SEED, CASE_SEED = 91, 5

# (n, p, g, K) of helpers.make_case and the create flags: the smallest shapes that cross every tiling remainder
CASES = {
    "A": ((37, 33, 3, 3), 0),             # fused; ragged n, P = 11
    "B": ((37, 33, 3, 7), UNFUSED),       # K <= 32 through the side-stream schedule
    "C": ((150, 90, 2, 40), 0),           # 64-wide: two row tiles, P = 45 crosses a 32-row loading tile
    "D": ((200, 90, 2, 66), 0),           # 128-wide
}
PATTERNS = ("random", "edges", "pairs", "none")


def make_mask(pattern, n, P, g, seed=17):
    """Boolean n x P x g mask (True = missing) of a named pattern."""
    mk = np.zeros((n, P, g), dtype=bool)
    if pattern == "none":
        return mk
    if pattern == "random":                                    # 15 % missing completely at random
        return np.random.default_rng(seed).random((n, P, g)) < 0.15
    if pattern == "edges":
        # the last shard has none; the others their two corner entries; shard 0 also one whole row and one column
        # with n - 2 missing; the inner columns of shard 1 (or, at g = 2, all of the last shard) have none
        for m in range(g - 1):
            mk[0, 0, m] = mk[n - 1, P - 1, m] = True
        mk[5, :, 0] = True
        mk[:, 2, 0] = True
        mk[[4, n - 3], 2, 0] = False
        assert mk[:, 2, 0].sum() == n - 2 and not mk[:, :, g - 1].any()
        return mk
    if pattern == "pairs":
        # rows 2r and 2r + 1 are the two normals of one Philox call: both missing, only the even, only the odd
        for m in range(g):
            for j in (0, P // 2, P - 1):
                mk[[2, 3], j, m] = True
                mk[6, j, m] = True
                mk[9, j, m] = True
                mk[[n - 2 - (n % 2), n - 1 - (n % 2)], j, m] = True      # the last full pair
                if n % 2:
                    mk[n - 1, j, m] = True                                 # the odd row out: n0 of a call alone
        return mk
    raise ValueError(pattern)


def impute_ref(Yd, mask, eta, Lambda, ps, normals):
    """The step in NumPy.  Yd, mask, normals n x P x g; eta n x K x g; Lambda P x K x g; ps P x 1 x g or P x g.
    Returns (Y_new, mu): the missing entries redrawn, the observed ones untouched; mu n x P x g everywhere."""
    ps = np.asarray(ps, dtype=np.float64).reshape(Lambda.shape[0], Lambda.shape[2])
    mu = np.einsum("ikm,jkm->ijm", eta, Lambda)
    return np.where(mask, mu + normals / np.sqrt(ps)[None, :, :], Yd), mu


def impute_naive(Yd, mask, eta, Lambda, ps, normals):
    """impute_ref as a triple loop with a k-ascending dot product."""
    n, P, g = Yd.shape
    K = Lambda.shape[1]
    ps = np.asarray(ps, dtype=np.float64).reshape(P, g)
    Y, mu = np.array(Yd, dtype=np.float64), np.zeros((n, P, g))
    for m in range(g):
        for j in range(P):
            for i in range(n):
                s = 0.0
                for k in range(K):
                    s += eta[i, k, m] * Lambda[j, k, m]
                mu[i, j, m] = s
                if mask[i, j, m]:
                    Y[i, j, m] = s + normals[i, j, m] / np.sqrt(ps[j, m])
    return Y, mu


def magnitude(mask, eta, Lambda, ps, normals):
    """sum_k |eta_ik lambda_jk| + |z| / sqrt(ps_j): what test 1's bar is relative to."""
    ps = np.asarray(ps, dtype=np.float64).reshape(Lambda.shape[0], Lambda.shape[2])
    return np.einsum("ikm,jkm->ijm", np.abs(eta), np.abs(Lambda)) + np.abs(normals) / np.sqrt(ps)[None, :, :]


def yy_ref(Y, mask):
    """The yy rule, P x g: a column with a missing entry gets (sum over its observed entries) + (sum over its
    missing ones), any other the plain sum of squares."""
    obs = np.where(mask, 0.0, Y * Y).sum(axis=0)
    return obs + np.where(mask, Y * Y, 0.0).sum(axis=0)


def impute_normals(seed, n, P, shards, it):
    """n x P x len(shards) normals of the step at iteration `it`, from the host restatement of the device's
    Philox stream: variate (j, i) of global shard mg at fill(site 13, shard mg, width n)[j n + i]."""
    from oracle import philox_ref as R
    out = np.empty((n, P, len(shards)))
    for a, mg in enumerate(shards):
        v = R.fill("normal", P * n, seed=seed, site=SITE_IMPUTE, shard=int(mg), iteration=int(it), width=n)
        out[:, :, a] = np.asarray(v, dtype=np.float64).reshape(P, n).T
    return out


# ---- test 9, "it imputes": one fixed data set, partition, initial state and 15 % MCAR mask; the reference chain is
# oracle.vectorised.gibbs_iteration followed by the step in NumPy (tests/golden/make_missing.py records its scores)
CHAIN = dict(n=150, p=60, k0=3, sparsity=0.3, g=3, K=3, rho=0.5, burnin=150, mcmc=300, thin=3, init_seed=41,
             mask_seed=100, nmiss=1347, seeds=(101, 102, 103, 104, 105, 106, 107, 108))


def chain_case():
    """The fixed start of the imputation chains: Y with its NaNs, the held-back truth, the partition, the
    standardised data (missing entries 0), the mask and the initial state, all from CHAIN's seeds."""
    import oracle
    from oracle import dc_oracle as F
    C = CHAIN
    Yfull, _ = oracle.synth.make_data(C["n"], C["p"], k0=C["k0"], sparsity=C["sparsity"])
    hole = np.random.default_rng(C["mask_seed"]).random(Yfull.shape) < 0.15
    Y = np.where(hole, np.nan, Yfull)
    hyper = F.Hyper()
    n, p, g, K = C["n"], C["p"], C["g"], C["K"]
    init = oracle.DrawSource(C["init_seed"], n, p, g, K, hyper).init()
    P = p // g
    st = F.initialise(n, P, K, g, C["rho"], hyper, init)
    cols = np.asarray(init.varind)
    Yp = np.stack([Y[:, cols[m * P:(m + 1) * P]] for m in range(g)], axis=2)           # n x P x g, NaN = missing
    mask = np.isnan(Yp)
    nobs = n - mask.sum(axis=0)
    mean = np.where(mask, 0.0, Yp).sum(axis=0) / nobs
    dev = np.where(mask, 0.0, Yp - mean)
    sd = np.sqrt((dev * dev).sum(axis=0) / (nobs - 1))
    truth = (np.stack([Yfull[:, cols[m * P:(m + 1) * P]] for m in range(g)], axis=2) - mean) / sd
    return dict(Y=Y, Yd=dev / sd, mask=mask, truth=truth, st=st, init=init, hyper=hyper, n=n, p=p, P=P, g=g, K=K,
                rho=C["rho"])


def score(mean, sd_total, truth, mask):
    """(r, c): the RMSE of the posterior mean over the missing entries against the held-back truth, divided by the
    RMSE of column-mean imputation (0 in observed-entry standardised units); the share of missing entries with
    |mean - truth| <= 2 sd_total."""
    e = (mean - truth)[mask]
    r = float(np.sqrt(np.mean(e * e)) / np.sqrt(np.mean(truth[mask] ** 2)))
    return r, float(np.mean(np.abs(e) <= 2.0 * sd_total[mask]))


def reference_chain(cc, seed):
    """One reference chain from chain_case()'s start: returns (r, c)."""
    import oracle
    from oracle import vectorised as V
    C = CHAIN
    st = cc["st"].copy()
    src = oracle.DrawSource(seed, cc["n"], cc["p"], cc["g"], cc["K"], cc["hyper"])
    rng = np.random.default_rng([seed, 13])
    Y, mask = np.array(cc["Yd"], order="F"), cc["mask"]
    s1, s2, sv, cnt = np.zeros(Y.shape), np.zeros(Y.shape), np.zeros(Y.shape[1:]), 0
    for it in range(1, C["burnin"] + C["mcmc"] + 1):
        V.gibbs_iteration(st, Y, cc["rho"], cc["hyper"], src.iteration(it))
        Y, mu = impute_ref(Y, mask, st.eta, st.Lambda, st.ps, rng.standard_normal(Y.shape))
        if it > C["burnin"] and it % C["thin"] == 0:
            s1 += mu
            s2 += mu * mu
            sv += 1.0 / st.ps[:, 0, :]
            cnt += 1
    m = s1 / cnt
    tot = sv / cnt + np.maximum(s2 / cnt - m * m, 0.0)
    return score(m, np.sqrt(tot), cc["truth"], mask)
