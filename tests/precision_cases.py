"""Shared setup of the precision-draw tests (test_precision_host.py, test_gpu_precision_draws.py): a NumPy
restatement of the nested Woodbury recursion of csrc/precision.hip, the dense reference with its condition
number, the derived bounds, a short injected chain with the precision probes set before it runs, and the
two-rank loopback harness (probe_cases.loopback_probed with set_precision_probes)."""
import threading

import numpy as np
from scipy.linalg import solve_triangular

import probe_cases as pc
from helpers import make_case, stacked_draws, state_dict

EPS = pc.EPS


def woodbury(V, Lambda, omega, rho):
    """(V' Sigma(s)^-1 V, log det Sigma(s)) by the recursion: per shard one weighted Gram of [L_m | V_m], a
    K x K Cholesky and two triangular solves, then one more K x K Cholesky.  Lambda P x K x g, omega P x g,
    V p x nv (shard m owns rows m P .. (m + 1) P)."""
    P, K, g = Lambda.shape
    V = V.reshape(P * g, -1)
    nv = V.shape[1]
    a = 1.0 - rho
    F, H, q, ld = np.zeros((K, nv)), np.zeros((K, K)), np.zeros((nv, nv)), 0.0
    for m in range(g):
        L, Vm, w = Lambda[:, :, m], V[m * P:(m + 1) * P], 1.0 / omega[:, m]
        G, U, d = L.T @ (w[:, None] * L), L.T @ (w[:, None] * Vm), Vm.T @ (w[:, None] * Vm)
        R = np.linalg.cholesky(np.eye(K) + a * G)
        T = solve_triangular(R, U, lower=True)
        q += d - a * T.T @ T
        F += solve_triangular(R, T, lower=True, trans="T")
        H += solve_triangular(R, solve_triangular(R, G, lower=True), lower=True, trans="T")
        ld += np.log(omega[:, m]).sum() + 2.0 * np.log(R.diagonal()).sum()
    R = np.linalg.cholesky(np.eye(K) + rho * 0.5 * (H + H.T))
    T = solve_triangular(R, F, lower=True)
    return q - rho * T.T @ T, ld + 2.0 * np.log(R.diagonal()).sum()


def dense(V, Lambda, omega, rho):
    """(Q_dense = V' solve(Sigma(s), V), slogdet, kappa = cond_2 Sigma(s)) from the oracle's Sigma(s)."""
    Sig = pc.sample_sigma(Lambda, omega, rho)
    V = V.reshape(Sig.shape[0], -1)
    sign, ld = np.linalg.slogdet(Sig)
    assert sign > 0
    return V.T @ np.linalg.solve(Sig, V), ld, np.linalg.cond(Sig)


def bounds(Qd, kappa, P, K, g, nv):
    """The issue's bounds: per entry 4 (P + K + g + nv) eps kappa sqrt(Q_aa Q_bb), and for the log det
    4 (P + K + g) p eps kappa (delta log det = tr(Sigma^-1 delta Sigma)).  Both the recursion and the dense
    solve are accurate to first order in eps kappa only."""
    dq = np.sqrt(np.abs(Qd.diagonal()))
    return 4.0 * (P + K + g + nv) * EPS * kappa * np.outer(dq, dq), 4.0 * (P + K + g) * (P * g) * EPS * kappa


def ratios(Q, ld, V, st, rho):
    """(max |Q - Q_dense| / bound, |ld - ld_dense| / bound, kappa) of one draw against the state st."""
    P, K, g = st["Lambda"].shape
    Qd, ldd, kappa = dense(V, st["Lambda"], st["omega"], rho)
    bq, bl = bounds(Qd, kappa, P, K, g, Qd.shape[0])
    rq = float(np.max(np.abs(Q - Qd) / np.where(bq > 0, bq, 1.0))) if Qd.size else 0.0
    return rq, abs(ld - ldd) / bl, kappa


def run_precision(dcfm, shape, V, capacity=None, states=True, keep=False, case_seed=21, rho=0.5, probes=None, **kw):
    """The injected chain of `shape` = (n, p, g, K) at rho with precision probes V (and V' Sigma V probes
    `probes`), one iteration per run call (`states`: the state read back after every saved one; else one
    call).  Returns {"Q", "logdet", "probe" (probe_draws), "states", "rho", "smp" (open, with keep)}."""
    n, p, g, K = shape
    c = make_case(n, p, g, K, seed=case_seed, k0=4, rho=rho)
    smp = pc.start(dcfm, c, g, K, **kw)
    try:
        if V is not None:
            smp.set_precision_probes(V, capacity)
        if probes is not None:
            smp.set_probes(probes)
        sts = []
        if not states:
            smp.run(1, pc.N)
        for it in range(1, pc.N + 1 if states else 0):
            smp.run(it, 1)
            if it in pc.SAVED:
                sts.append(smp.get_state(("Lambda", "omega")))
        Q, ld = smp.precision_draws()
        out = {"Q": Q, "logdet": ld, "probe": smp.probe_draws(), "states": sts, "rho": c["rho"],
               "smp": smp if keep else None}
    finally:
        if not keep:
            smp.close()
    return out


def oracle_states(shape, rho=0.5, case_seed=21):
    """The saved states (Lambda, omega) of the same injected chain by the oracle (CPU)."""
    from oracle import dc_oracle as F
    n, p, g, K = shape
    c = make_case(n, p, g, K, seed=case_seed, k0=4, rho=rho)
    st, out = c["st"].copy(), []
    for it in range(1, pc.N + 1):
        F.gibbs_iteration(st, c["Yd"], rho, c["hyper"], c["src"].iteration(it))
        if it in pc.SAVED:
            out.append({"Lambda": st.Lambda.copy(), "omega": st.omega.copy()})
    return out


def loopback_precision(dcfm, V, n=60, p=400, g=4, K=5):
    """Two loopback ranks of one injected chain on one device with precision probes V set before the run;
    each rank's precision_draws() (collective) from its own thread.  Returns (the two results, the case)."""
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
            smp.set_precision_probes(V)

        def run(r):
            try:
                smps[r].run(1, pc.N)
                out[r] = smps[r].precision_draws()
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
