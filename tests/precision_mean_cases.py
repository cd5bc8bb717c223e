"""Shared setup of the precision-mean tests (test_precision_mean_host.py, test_gpu_precision_mean.py): NumPy
restatements of the factor forms of csrc/precision_mean.hip, the dense reference (1/effsamp) sum_s inv(Sigma(s))
with every sample's condition number and the entrywise bound, and the short injected chain of probe_cases
with DCFM_FLAG_PRECISION_MEAN set."""
import numpy as np

import probe_cases as pc
from helpers import make_case

EPS = pc.EPS


def factors(Lambda, omega, rho):
    """(ps, A, Gamma) of one sample, Lambda P x K x g and omega P x g: ps = 1 / omega (p,), and the p x K
    panels A_m = sqrt(1 - rho) Omega_m^-1 L_m C_m (C_m C_m' = B_m^-1) and Gamma_m = sqrt(rho) Omega_m^-1 L_m
    B_m^-1 E (E E' = S^-1), with G_m = L_m' Omega_m^-1 L_m, B_m = I + (1 - rho) G_m, H_m = B_m^-1 G_m and
    S = I + rho sum_m H_m (the shards in shard order), so that
        inv(Sigma(s))_ab = [a == b] ps_a - [a, b in one shard] A_a . A_b - Gamma_a . Gamma_b."""
    P, K, g = Lambda.shape
    a = 1.0 - rho
    ps = (1.0 / omega).T.reshape(-1)
    A, M, H = np.zeros((P * g, K)), np.zeros((P * g, K)), np.zeros((K, K))
    for m in range(g):
        X = Lambda[:, :, m] / omega[:, m, None]               # Omega^-1 L
        G = Lambda[:, :, m].T @ X
        Binv = np.linalg.inv(np.eye(K) + a * G)
        Binv = 0.5 * (Binv + Binv.T)
        H += Binv @ G
        M[m * P:(m + 1) * P] = X @ Binv
        A[m * P:(m + 1) * P] = np.sqrt(a) * (X @ np.linalg.cholesky(Binv))
    Sinv = np.linalg.inv(np.eye(K) + rho * 0.5 * (H + H.T))
    return ps, A, np.sqrt(rho) * (M @ np.linalg.cholesky(0.5 * (Sinv + Sinv.T)))


def panels(Lambda, omega, rho):
    """(ps, Left, Right), the asymmetric two-panel form the device accumulates (inverses only, no Cholesky):
    Left_m = Omega_m^-1 L_m B_m^-1 [rho S^-1 | (1 - rho) I], Right_m = Omega_m^-1 L_m [B_m^-1 | I], each p x 2K
    with the cross-shard (Gamma) half first."""
    P, K, g = Lambda.shape
    a = 1.0 - rho
    ps = (1.0 / omega).T.reshape(-1)
    X, M, H = np.zeros((P * g, K)), np.zeros((P * g, K)), np.zeros((K, K))
    for m in range(g):
        X[m * P:(m + 1) * P] = Lambda[:, :, m] / omega[:, m, None]
        G = Lambda[:, :, m].T @ X[m * P:(m + 1) * P]
        Binv = np.linalg.inv(np.eye(K) + a * G)
        H += Binv @ G
        M[m * P:(m + 1) * P] = X[m * P:(m + 1) * P] @ Binv
    Sinv = np.linalg.inv(np.eye(K) + rho * H)
    return ps, np.hstack([rho * (M @ Sinv), a * M]), np.hstack([M, X])


def from_panels(ps, Left, Right, P):
    """inv(Sigma(s)) from (ps, Left, Right): Left = Right = [Gamma | A] for the symmetric form.  The lower
    triangle is formed and mirrored, as the device stores it."""
    p, K = Left.shape[0], Left.shape[1] // 2
    same = (np.arange(p)[:, None] // P) == (np.arange(p)[None, :] // P)
    T = np.diag(ps) - Left[:, :K] @ Right[:, :K].T - np.where(same, Left[:, K:] @ Right[:, K:].T, 0.0)
    return np.tril(T) + np.tril(T, -1).T


def sample_precision(Lambda, omega, rho):
    """inv(Sigma(s)) by the A / Gamma form."""
    ps, A, Gm = factors(Lambda, omega, rho)
    F = np.hstack([Gm, A])
    return from_panels(ps, F, F, Lambda.shape[0])


def dense_mean(states, rho, effsamp):
    """{"T": (1/effsamp) sum_s inv(Sigma(s)) from the oracle's dense Sigma(s) (probe_cases.sample_sigma),
    "kappa": cond_2 Sigma(s) of every sample, "bound": the entrywise bound (1/effsamp) sum_s
    4 (P + 2K + g) eps kappa_s sqrt(Theta(s)_aa Theta(s)_bb) -- precision_cases.bounds averaged; the factor
    form and the dense inverse are both accurate to first order in eps kappa only}."""
    P, K, g = states[0]["Lambda"].shape
    T, bound, kappa = np.zeros((P * g, P * g)), np.zeros((P * g, P * g)), []
    for st in states:
        Sig = pc.sample_sigma(st["Lambda"], st["omega"], rho)
        Ti = np.linalg.inv(Sig)
        Ti = 0.5 * (Ti + Ti.T)
        kappa.append(float(np.linalg.cond(Sig)))
        dq = np.sqrt(np.abs(Ti.diagonal()))
        T += Ti
        bound += 4.0 * (P + 2 * K + g) * EPS * kappa[-1] * np.outer(dq, dq)
    return {"T": T / effsamp, "kappa": kappa, "bound": bound / effsamp}


def ratio(T, ref):
    """max |T - T_ref| / bound."""
    return float(np.max(np.abs(T - ref["T"]) / ref["bound"]))


def run_mean(dcfm, shape, rho=0.5, states=True, case_seed=21, **kw):
    """The injected chain of probe_cases (burnin 1, mcmc 6, thin 2) on `shape` = (n, p, g, K) at rho with the
    precision mean on, one iteration per run call (`states`: Lambda and omega are read back after every
    saved one; else the chain runs in one call).  Returns {"T", "cols" (columns [37, 107) where p allows, else
    the last half), "c0", "states", "block"}."""
    n, p, g, K = shape
    c = make_case(n, p, g, K, seed=case_seed, k0=4, rho=rho)
    smp = pc.start(dcfm, c, g, K, precision_mean=True, **kw)
    try:
        sts = []
        if not states:
            smp.run(1, pc.N)
        for it in range(1, pc.N + 1 if states else 0):
            smp.run(it, 1)
            if it in pc.SAVED:
                sts.append(smp.get_state(("Lambda", "omega")))
        c0, nc = (37, 70) if p >= 107 else (p // 2, p - p // 2)
        return {"T": smp.get_precision_mean(), "cols": smp.get_precision_mean_cols(c0, nc), "c0": c0, "nc": nc,
                "states": sts, "block": smp.sigma_block(), "saved": smp.saved_samples()}
    finally:
        smp.close()
