"""Shared setup of the log-likelihood tests (test_loglik_host.py, test_gpu_loglik.py): a NumPy restatement of
the recursion of csrc/loglik.hip, the dense reference with its condition number, the bounds, a short injected
chain with set_loglik before it runs, and the two-rank loopback harness (precision_cases.loopback_precision
with set_loglik)."""
import threading

import numpy as np

import probe_cases as pc
from helpers import make_case, stacked_draws, state_dict

EPS = pc.EPS
# (n, p, g, K), rho: the states the recursion was checked on with the oracle's chain (kappa <= 2.8e2)
HOST_SHAPES = [((30, 60, 3, 3), 0.5), ((30, 60, 3, 3), 0.0), ((30, 60, 3, 3), 1.0), ((30, 21, 1, 1), 0.5),
               ((30, 60, 12, 2), 0.5), ((40, 90, 2, 40), 0.5), ((40, 99, 3, 33), 0.5), ((60, 400, 4, 5), 0.5),
               ((130, 74, 2, 5), 0.5)]


def rows(Yd):
    """The n x p rows y_i in Sigma(s)'s coordinates from Yd (n x P x g): shard m owns columns m P .. (m + 1) P."""
    Yd = np.asarray(Yd)
    return np.concatenate([Yd[:, :, m] for m in range(Yd.shape[2])], axis=1)


def recursion(Yd, Lambda, omega, rho):
    """(q (n,), log det Sigma(s)) exactly as loglik.hip states it: per shard T = Y Omega^-1 Lambda, s, G, B = I + a G,
    H = B^-1 G, F = T B^-1; then S = I + rho sym(H) and q_i = sum_m (s - a t.f) - rho u' S^-1 u."""
    P, K, g = Lambda.shape
    n = Yd.shape[0]
    a = 1.0 - rho
    U, H, q, ld = np.zeros((n, K)), np.zeros((K, K)), np.zeros(n), 0.0
    for m in range(g):
        L, Y, w = Lambda[:, :, m], Yd[:, :, m], 1.0 / omega[:, m]
        T = (Y * w) @ L
        s = (Y * Y) @ w
        G = L.T @ (w[:, None] * L)
        Binv = np.linalg.inv(np.eye(K) + a * G)
        F = T @ Binv.T
        q += s - a * np.einsum("ik,ik->i", T, F)
        U += F
        H += Binv @ G
        ld += np.log(omega[:, m]).sum() + np.linalg.slogdet(np.eye(K) + a * G)[1]
    S = np.eye(K) + rho * 0.5 * (H + H.T)
    q -= rho * np.einsum("ik,ik->i", U, np.linalg.solve(S, U.T).T)
    return q, ld + np.linalg.slogdet(S)[1]


def dense(Yd, Lambda, omega, rho):
    """(q_dense, slogdet, kappa = cond_2 Sigma(s)) from the oracle's Sigma(s) by a dense solve."""
    Sig = pc.sample_sigma(Lambda, omega, rho)
    Yr = rows(Yd)
    sign, ld = np.linalg.slogdet(Sig)
    assert sign > 0
    return np.einsum("ij,ji->i", Yr, np.linalg.solve(Sig, Yr.T)), ld, np.linalg.cond(Sig)


def bounds(qd, kappa, P, K, g):
    """Per row 4 (P + K + g + 1) eps kappa q_dense,i (the precision draws' bound with one probe), and for the log
    det 4 (P + K + g) p eps kappa (precision_cases.bounds).  Both sides are first order in eps kappa."""
    return 4.0 * (P + K + g + 1) * EPS * kappa * np.abs(qd), 4.0 * (P + K + g) * (P * g) * EPS * kappa


def ratios(q, ld, Yd, st, rho):
    """(max |q - q_dense| / bound, |ld - ld_dense| / bound, kappa) of one draw against the state st."""
    P, K, g = st["Lambda"].shape
    qd, ldd, kappa = dense(Yd, st["Lambda"], st["omega"], rho)
    bq, bl = bounds(qd, kappa, P, K, g)
    return float(np.max(np.abs(q - qd) / bq)), abs(ld - ldd) / bl, kappa


def assert_draw(q, ld, Yd, st, rho, what, frac=1.0):
    rq, rl, kappa = ratios(q, ld, Yd, st, rho)
    print(f"{what}: kappa {kappa:.3e}, q max err / bound {rq:.4f}, log det err / bound {rl:.5f}")
    assert np.all(np.isfinite(q)) and np.isfinite(ld)
    assert kappa <= 1e6, f"{what}: kappa {kappa:.3e}"
    assert rq <= frac, f"{what}: q is {rq:.3f} of its bound"
    assert rl <= frac, f"{what}: log det is {rl:.3f} of its bound"


def run_loglik(dcfm, shape, capacity=None, states=True, keep=False, case_seed=21, rho=0.5, probes=None,
               precision_rows=0, on=True, **kw):
    """The injected chain of `shape` = (n, p, g, K) at rho with set_loglik(capacity) (`on`), one iteration per
    run call (`states`: the state read back after every saved one; else one call).  `precision_rows` > 0: the
    first rows of get_data() as precision probes on the same chain; `probes`: a V' Sigma V block.  Returns
    {"ll", "maha", "logdet", "Q", "qlogdet" (precision_draws), "probe", "states", "Yd", "rho", "smp"}."""
    n, p, g, K = shape
    c = make_case(n, p, g, K, seed=case_seed, k0=4, rho=rho)
    smp = pc.start(dcfm, c, g, K, **kw)
    try:
        if on:
            smp.set_loglik(capacity)
        if precision_rows:
            smp.set_precision_probes(rows(smp.get_data())[:precision_rows].T)
        if probes is not None:
            smp.set_probes(probes)
        sts = []
        if not states:
            smp.run(1, pc.N)
        for it in range(1, pc.N + 1 if states else 0):
            smp.run(it, 1)
            if it in pc.SAVED:
                sts.append(smp.get_state(("Lambda", "omega")))
        ll, maha, ld = smp.loglik_draws(parts=True)
        Q, qld = smp.precision_draws()
        out = {"ll": ll, "maha": maha, "logdet": ld, "Q": Q, "qlogdet": qld, "probe": smp.probe_draws(),
               "states": sts, "Yd": c["Yd"], "rho": c["rho"], "smp": smp if keep else None}
    finally:
        if not keep:
            smp.close()
    return out


def loopback_loglik(dcfm, n=60, p=400, g=4, K=5):
    """Two loopback ranks of one injected chain on one device with set_loglik before the run; each rank's
    loglik_draws(parts=True) (collective) from its own thread.  Returns (the two results, the case)."""
    n_r = 2
    c = make_case(n, p, g, K, seed=23, k0=4)
    G = g // n_r
    draws = stacked_draws(c["src"], 1, pc.N)
    smps = [dcfm.Sampler(c["n"], c["P"], g, K, c["rho"], pc.BURNIN, pc.MCMC, pc.THIN, inject_draws=True,
                         nranks=n_r, rank=r, device=0) for r in range(n_r)]
    out, errs = [None] * n_r, []
    try:
        dcfm.Sampler.comm_loopback(smps)
        for r, smp in enumerate(smps):
            smp.set_data(c["Yd"][:, :, r * G:(r + 1) * G])
            st = state_dict(c["st"], r * G, G)
            smp.set_state({f: st[f] for f in st if f != "eta"})
            smp.set_draws(draws, 1, pc.N)
            smp.set_loglik()

        def run(r):
            try:
                smps[r].run(1, pc.N)
                out[r] = smps[r].loglik_draws(parts=True)
            except Exception as e:                                        # surfaced below
                errs.append(e)

        ths = [threading.Thread(target=run, args=(r,)) for r in range(n_r)]
        for t in ths:
            t.start()
        for t in ths:
            t.join(timeout=100)
        assert not any(t.is_alive() for t in ths), "a rank did not finish"
        assert not errs, errs
    finally:
        for smp in smps:
            smp.close()
    return out, c
