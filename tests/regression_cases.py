"""Shared setup of the regression tests (test_regression_host.py, test_gpu_regression.py): the dense NumPy
reference of the per-sample coefficients B(s)[O] = solve(Sigma_OO(s), Sigma_OR(s)), residual covariance C(s) =
Sigma_RR - Sigma_RO B(s)[O] and R2_j(s) = 1 - C_jj / Sigma_{r_j r_j} from the oracle's dense Sigma(s), with every
sample's condition number and the entrywise bound; the panel restatement of csrc/regression.hip built from
precision_mean_cases.panels; and the short injected chain of probe_cases with DCFM_FLAG_REGRESSION set."""
import numpy as np

import precision_mean_cases as mc
import probe_cases as pc
from helpers import make_case

EPS = pc.EPS

# ((n, p, g, K), rho): the shapes of partial_corr_cases.SWEEP that take a path of their own in regression.hip
CASES = [
    ((30, 48, 4, 5), 0.5),         # four shards in one 16-row tile, K odd
    ((30, 36, 3, 1), 0.5),         # K = 1
    ((24, 120, 20, 2), 0.5),       # P = 6: several shards in a 16-row tile
    ((24, 130, 2, 4), 0.5),        # P = 65: a shard edge off the tile edge
    ((37, 300, 3, 7), 0.0),        # no G half
    ((37, 300, 3, 7), 0.5),
    ((37, 300, 3, 7), 1.0),        # no A half
    ((64, 384, 3, 30), 0.5),       # P = 128, c3's K
    ((50, 128, 2, 32), 0.5),       # K = 32
    ((40, 99, 3, 33), 0.5),        # wide layout
    ((140, 256, 2, 128), 0.5),     # K = 128: the LDS limit of the panel stage
]
SETS = ("one", "five", "wide")
FIELDS = ("coef", "coef_m2", "rcov", "rcov_m2", "r2", "r2_m2")


def response_set(p, which):
    """The three response sets of a shape: one response; five with three in the first shard; min(32, p // 3)
    spread over the shards, listed in descending order (R need not be sorted)."""
    if which == "one":
        return np.array([p - 2], dtype=np.int64)
    if which == "five":
        return np.array([0, 1, 2, p // 2, p - 1], dtype=np.int64)
    q = min(32, p // 3)
    return ((np.arange(q, dtype=np.int64) * p) // q)[::-1].copy()


def _moments(Bs, Cs, Rs):
    S = len(Bs)
    return {"coef": sum(Bs) / S, "coef_m2": sum(B * B for B in Bs) / S, "rcov": sum(Cs) / S,
            "rcov_m2": sum(C * C for C in Cs) / S, "r2": sum(Rs) / S, "r2_m2": sum(r * r for r in Rs) / S}


def dense_ref(states, rho, R):
    """The six moments (population form, 1 / S) from the definition, on the oracle's dense Sigma(s)
    (probe_cases.sample_sigma), plus "kappa" (cond_2 Sigma(s) of every sample), "bound" (p x q: (1 / S) sum_s
    4 (P + 2 K + g) eps kappa_s sqrt(Theta(s)_aa C(s)_jj), the entrywise bound on coef) and "var_*" (the population
    variances of the three quantities)."""
    P, K, g = states[0]["Lambda"].shape
    p, R = P * g, np.asarray(R)
    O = np.setdiff1d(np.arange(p), R)
    Bs, Cs, Rs, kappa, bound = [], [], [], [], np.zeros((p, R.size))
    for st in states:
        Sig = pc.sample_sigma(st["Lambda"], st["omega"], rho)
        B = np.zeros((p, R.size))
        B[O] = np.linalg.solve(Sig[np.ix_(O, O)], Sig[np.ix_(O, R)])
        C = Sig[np.ix_(R, R)] - Sig[np.ix_(R, O)] @ B[O]
        C = 0.5 * (C + C.T)
        kappa.append(float(np.linalg.cond(Sig)))
        th = np.abs(np.linalg.inv(Sig).diagonal())
        bound += 4.0 * (P + 2 * K + g) * EPS * kappa[-1] * np.sqrt(np.outer(th, np.abs(C.diagonal())))
        Bs.append(B)
        Cs.append(C)
        Rs.append(1.0 - C.diagonal() / Sig.diagonal()[R])
    out = _moments(Bs, Cs, Rs)
    out.update(kappa=kappa, bound=bound / len(states))
    for f, m2 in (("coef", "coef_m2"), ("rcov", "rcov_m2"), ("r2", "r2_m2")):
        out["var_" + f] = out[m2] - out[f] * out[f]
    return out


def panel_sample(Lambda, omega, rho, R):
    """(B(s), C(s), R2(s)) by the panel form of csrc/regression.hip: T = Theta[:, R] from the four panels, Q its
    symmetrised response rows, C = inv(Q) with the lower triangle mirrored, B = -T C with the response rows 0."""
    P = Lambda.shape[0]
    ps, Left, Right = mc.panels(Lambda, omega, rho)
    p, K, R = Left.shape[0], Left.shape[1] // 2, np.asarray(R)
    same = (np.arange(p)[:, None] // P) == (R[None, :] // P)
    T = -Left[:, :K] @ Right[R, :K].T - np.where(same, Left[:, K:] @ Right[R, K:].T, 0.0)
    T[R, np.arange(R.size)] += ps[R]
    C = np.linalg.inv(0.5 * (T[R] + T[R].T))
    C = np.tril(C) + np.tril(C, -1).T
    B = -T @ C
    B[R] = 0.0
    lam = np.transpose(Lambda, (2, 0, 1)).reshape(p, K)          # row a = m P + j
    v = np.einsum("ak,ak->a", lam, lam) + np.asarray(omega).T.reshape(-1)
    return B, C, 1.0 - C.diagonal() / v[R]


def panel_ref(states, rho, R):
    """The six moments by the panel restatement."""
    parts = [panel_sample(st["Lambda"], st["omega"], rho, R) for st in states]
    return _moments([x[0] for x in parts], [x[1] for x in parts], [x[2] for x in parts])


def read_raw(smp):
    """Sampler.regression_raw() as a dict of FIELDS plus "count"."""
    out = dict(zip(FIELDS + ("count",), smp.regression_raw()))
    return out


def run_reg(dcfm, shape, rho, R, states=True, case_seed=21, **kw):
    """The injected chain of probe_cases (burnin 1, mcmc 6, thin 2) on `shape` = (n, p, g, K) at rho with the
    regression on R, one iteration per run call (`states`: Lambda and omega are read back after every saved one;
    else the chain runs in one call).  Returns read_raw's dict plus "states" and "block"."""
    n, p, g, K = shape
    c = make_case(n, p, g, K, seed=case_seed, k0=4, rho=rho)
    smp = pc.start(dcfm, c, g, K, regression=True, **kw)
    try:
        smp.set_regression(R)
        sts = []
        if not states:
            smp.run(1, pc.N)
        for it in range(1, pc.N + 1 if states else 0):
            smp.run(it, 1)
            if it in pc.SAVED:
                sts.append(smp.get_state(("Lambda", "omega")))
        out = read_raw(smp)
        out.update(states=sts, block=smp.sigma_block())
        return out
    finally:
        smp.close()
