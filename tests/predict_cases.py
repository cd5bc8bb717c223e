"""Shared setup of the conditional-prediction tests (test_predict_host.py, test_gpu_predict.py): a NumPy
restatement of the recursion of csrc/predict.hip, the dense Gaussian conditional as reference with the condition
number of Sigma_AA(s), the bounds, mask builders, and the stepped injected chain with the prediction set before
it runs (the schedule of probe_cases, the state and the read-out fetched at every saved iteration)."""
import numpy as np

import probe_cases as pc
from helpers import make_case

EPS = pc.EPS
MASKS = ("random", "shard_off", "shard_on", "single", "empty", "full")


def mask(kind, P, g, seed=3):
    """A 0 / 1 mask over the p = P g variables (shard m owns rows m P .. (m + 1) P): `random` about 60 %
    observed, `shard_off` random with the last shard fully unobserved, `shard_on` random with the first shard
    fully observed, `single` one observed variable, `empty`, `full`."""
    p = P * g
    rng = np.random.default_rng(seed)
    ob = rng.random(p) < 0.6
    if kind == "shard_off":
        ob[(g - 1) * P:] = False
    elif kind == "shard_on":
        ob[:P] = True
    elif kind == "single":
        ob[:] = False
        ob[(5 * p) // 7] = True
    elif kind == "empty":
        ob[:] = False
    elif kind == "full":
        ob[:] = True
    else:
        assert kind == "random", kind
    return ob.astype(np.uint8)


def new_rows(p, T, seed=9):
    """p x T seeded normals; from three columns on, column 1 is all zero."""
    Y = np.random.default_rng(seed).standard_normal((p, T))
    if T >= 3:
        Y[:, 1] = 0.0
    return Y


def recursion(Ystar, obs, Lambda, omega, rho):
    """(yhat p x T, cv p, q T, ld) by the recursion the device runs: the masked weighted Gram per shard, the K x K
    inverses, the coefficients t_m and M_m, and one product per loading row.  Lambda P x K x g, omega P x g."""
    P, K, g = Lambda.shape
    ob = np.asarray(obs).astype(bool).reshape(g, P)
    Ys = np.where(ob.reshape(-1)[:, None], np.asarray(Ystar, dtype=np.float64).reshape(P * g, -1), 0.0)
    T = Ys.shape[1]
    a, I = 1.0 - rho, np.eye(K)
    Hm, Fm, qs, ld = [], [], np.zeros(T), 0.0
    for m in range(g):
        L, Ym = Lambda[:, :, m], Ys[m * P:(m + 1) * P]
        w = np.where(ob[m], 1.0 / np.where(ob[m], omega[:, m], 1.0), 0.0)
        G, U, d = L.T @ (w[:, None] * L), L.T @ (w[:, None] * Ym), np.einsum("jt,j,jt->t", Ym, w, Ym)
        Bi = np.linalg.inv(I + a * G)
        Hm.append(Bi @ G)
        Fm.append(Bi @ U)
        qs += d - a * np.einsum("kt,kt->t", U, Fm[-1])
        ld += np.log(omega[ob[m], m]).sum() + np.linalg.slogdet(I + a * G)[1]
    H, F = sum(Hm), sum(Fm)
    S = I + rho * H
    R = np.linalg.inv(S)
    X = R @ F
    q = qs - rho * np.einsum("kt,kt->t", F, X)
    ld += np.linalg.slogdet(S)[1]
    c = F - rho * H @ X
    yhat, cv = np.zeros((P * g, T)), np.zeros(P * g)
    for m in range(g):
        tm = a * (Fm[m] - rho * Hm[m] @ X) + rho * c
        M = a * a * (Hm[m] - rho * Hm[m] @ R @ Hm[m]) + a * rho * (Hm[m] @ R + R @ Hm[m]) + rho * rho * R @ H
        L = Lambda[:, :, m]
        yhat[m * P:(m + 1) * P] = L @ tm
        cv[m * P:(m + 1) * P] = np.einsum("jk,kl,jl->j", L, I - M, L) + omega[:, m]
    return yhat, cv, q, ld


def dense(Ystar, obs, Lambda, omega, rho):
    """The dense Gaussian conditional of the oracle's Sigma(s): with C = Sigma - Omega, yhat = C[:, A]
    Sigma_AA^-1 y_A, cv_j = C_jj - C_jA Sigma_AA^-1 C_Aj + omega_j, q = y_A' Sigma_AA^-1 y_A, ld = log det
    Sigma_AA.  Returns {"yhat", "cv", "q", "ld", "kappa" (cond_2 Sigma_AA, 1 for an empty A), "diag" (Sigma_jj),
    "nobs", "z" (Sigma_AA^-1 y_A on A, else 0)}."""
    P, K, g = Lambda.shape
    p = P * g
    Sig = pc.sample_sigma(Lambda, omega, rho)
    om = np.asarray(omega).T.reshape(-1)                       # row m P + j
    C = Sig - np.diag(om)
    A = np.flatnonzero(np.asarray(obs).reshape(-1))
    Y = np.asarray(Ystar, dtype=np.float64).reshape(p, -1)
    T = Y.shape[1]
    out = {"diag": Sig.diagonal().copy(), "nobs": A.size, "z": np.zeros((p, T))}
    if A.size == 0:
        out.update(yhat=np.zeros((p, T)), cv=C.diagonal() + om, q=np.zeros(T), ld=0.0, kappa=1.0)
        return out
    SA = Sig[np.ix_(A, A)]
    z = np.linalg.solve(SA, Y[A])
    W = np.linalg.solve(SA, C[A, :])
    sign, ld = np.linalg.slogdet(SA)
    assert sign > 0
    out["z"][A] = z
    out.update(yhat=C[:, A] @ z, cv=C.diagonal() - np.einsum("aj,aj->j", C[A, :], W) + om,
               q=np.einsum("at,at->t", Y[A], z), ld=ld, kappa=np.linalg.cond(SA))
    return out


def bounds(d, P, K, g, T):
    """The bars of one sample, from the dense result d: with dim = P + K + g + T, per entry
    4 dim eps kappa sqrt(Sigma_jj q_t) for yhat (the scale is the Cauchy-Schwarz bound of |yhat_jt|),
    4 dim eps kappa Sigma_jj for cv, 4 dim eps kappa q_t for q and 4 (P + K + g) |A| eps kappa for the log det.
    Both the recursion and the dense solve are accurate to first order in eps kappa only."""
    c = 4.0 * (P + K + g + T) * EPS * d["kappa"]
    q = np.abs(d["q"])
    return {"yhat": c * np.sqrt(np.outer(d["diag"], q)), "cv": c * d["diag"], "q": c * q,
            "ld": 4.0 * (P + K + g) * d["nobs"] * EPS * d["kappa"]}


def _ratio(err, bar):
    """max err / bar; an entry with a zero bar must be exact."""
    err, bar = np.atleast_1d(np.abs(err)), np.atleast_1d(bar)
    if err.size == 0:
        return 0.0
    r = np.where(bar > 0, err / np.where(bar > 0, bar, 1.0), np.where(err == 0, 0.0, np.inf))
    return float(np.max(r))


def ratios(yhat, cv, q, ld, d, b):
    """max |value - dense| / bar of one sample's four outputs."""
    return {"yhat": _ratio(yhat - d["yhat"], b["yhat"]), "cv": _ratio(cv - d["cv"], b["cv"]),
            "q": _ratio(q - d["q"], b["q"]), "ld": _ratio(ld - d["ld"], b["ld"])}


class Running:
    """The running average of the dense per-sample values and of their bars: what the accumulated read-outs are
    compared with.  bar = the average of the per-sample bars + count eps max |term|; for m2 the per-sample bar is
    2 |yhat_dense| bar(yhat) + bar(yhat)^2."""

    def __init__(self):
        self.n = 0
        self.sum, self.bar, self.top = {}, {}, {}

    def add(self, d, b):
        terms = {"mean": (d["yhat"], b["yhat"]), "m2": (d["yhat"] ** 2, 2.0 * np.abs(d["yhat"]) * b["yhat"] + b["yhat"] ** 2),
                 "cvar": (d["cv"], b["cv"])}
        for f, (v, bar) in terms.items():
            self.sum[f] = self.sum.get(f, 0.0) + v
            self.bar[f] = self.bar.get(f, 0.0) + bar
            self.top[f] = max(self.top.get(f, 0.0), float(np.max(np.abs(v))) if v.size else 0.0)
        self.n += 1

    def ratios(self, mean, m2, cvar):
        got = {"mean": mean, "m2": m2, "cvar": cvar}
        return {f: _ratio(got[f] - self.sum[f] / self.n, self.bar[f] / self.n + self.n * EPS * self.top[f])
                for f in got}


def run_predict(dcfm, shape, Ynew, obs, capacity=None, states=True, keep=False, case_seed=21, rho=0.5, setup=None,
                **kw):
    """The injected chain of `shape` = (n, p, g, K) at rho with the prediction of (Ynew, obs) set before it runs
    (Ynew None: not set), one iteration per run call (`states`: the state and predict_raw() read back after every
    saved one; else one call).  `setup(smp)` runs before the prediction is set.  Returns {"raw" (the last
    predict_raw()), "reads" (one per saved iteration), "states", "rho", "smp" (open, with keep)}."""
    n, p, g, K = shape
    c = make_case(n, p, g, K, seed=case_seed, k0=4, rho=rho)
    smp = pc.start(dcfm, c, g, K, **kw)
    try:
        if setup is not None:
            setup(smp)
        if obs is not None:
            smp.set_predict(Ynew, obs, capacity)
        sts, reads = [], []
        if not states:
            smp.run(1, pc.N)
        for it in range(1, pc.N + 1 if states else 0):
            smp.run(it, 1)
            if it in pc.SAVED:
                sts.append(smp.get_state(("Lambda", "omega")))
                reads.append(smp.predict_raw())
        out = {"raw": smp.predict_raw(), "reads": reads, "states": sts, "rho": c["rho"], "smp": smp if keep else None}
    finally:
        if not keep:
            smp.close()
    return out


def raw_bytes(raw):
    """The bytes of a predict_raw() tuple, for the bitwise comparisons."""
    return b"".join(np.ascontiguousarray(a).tobytes() for a in raw[:5]) + bytes([raw[5]])
