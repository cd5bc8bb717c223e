"""Shared setup of the partial-correlation tests (test_partial_corr_host.py, test_gpu_partial_corr.py): the dense
NumPy reference of the two moments of R(s)_ab = -Theta(s)_ab / sqrt(Theta(s)_aa Theta(s)_bb), Theta(s) the inverse
of the oracle's Sigma(s), with every sample's condition number and the entrywise bound; the scaled-panel
restatement of csrc/partial_corr.hip built from precision_mean_cases.panels; and the short injected chain of
probe_cases with DCFM_FLAG_PARTIAL_CORR set."""
import numpy as np

import precision_mean_cases as mc
import probe_cases as pc
from helpers import make_case

EPS = pc.EPS

# ((n, p, g, K), rho): what each shape covers on the device
SWEEP = [
    ((30, 48, 4, 5), 0.5),         # four shards in one partial tile, K odd
    ((30, 36, 3, 1), 0.5),         # K = 1
    ((24, 120, 20, 2), 0.5),       # P = 6, twenty shards in a tile: the per-pair mask
    ((24, 130, 2, 4), 0.5),        # P = 65: a shard edge off the tile edge, and a second tile row
    ((37, 300, 3, 7), 0.5),        # mixed tiles
    ((37, 300, 3, 7), 0.0),        # no G half
    ((37, 300, 3, 7), 1.0),        # no A half
    ((64, 384, 3, 30), 0.5),       # P = 128: pure cross and pure same-shard tiles, c3's K
    ((50, 128, 2, 32), 0.5),       # K = 32
    ((40, 99, 3, 33), 0.5),        # wide layout
    ((32, 1152, 9, 3), 0.5),       # crosses a supertile
    ((120, 200, 2, 100), 0.5),     # K = 100
    ((140, 256, 2, 128), 0.5),     # K = 128: the LDS limit of the panel stage
]


def sample_partial(Theta):
    """R = -Theta_ab / sqrt(Theta_aa Theta_bb) with an exact unit diagonal (diagnostics.partial_correlations'
    convention)."""
    s = np.sqrt(Theta.diagonal())
    R = -Theta / (s[:, None] * s[None, :])
    R[np.diag_indices_from(R)] = 1.0
    return R


def dense_moments(states, rho, effsamp):
    """{"PC": (1/effsamp) sum_s R(s), "PC2": (1/effsamp) sum_s R(s)^2, "var": the population variance of R(s) over
    the saved samples, "kappa": cond_2 Sigma(s) of every sample, "b": the bound (1/effsamp) sum_s 8 (P + 2K + g)
    eps kappa_s} with R(s) from np.linalg.inv of the oracle's dense Sigma(s) (probe_cases.sample_sigma).  b is
    twice the entrywise bound of precision_mean_cases.dense_mean after normalisation by sqrt(Theta_aa Theta_bb):
    the division adds the relative error of two diagonal entries to that of Theta_ab, and |R| <= 1."""
    P, K, g = states[0]["Lambda"].shape
    p = P * g
    S1, S2, kappa = np.zeros((p, p)), np.zeros((p, p)), []
    for st in states:
        Sig = pc.sample_sigma(st["Lambda"], st["omega"], rho)
        Ti = np.linalg.inv(Sig)
        R = sample_partial(0.5 * (Ti + Ti.T))
        kappa.append(float(np.linalg.cond(Sig)))
        S1 += R
        S2 += R * R
    ns = len(states)
    m = S1 / ns
    return {"PC": S1 / effsamp, "PC2": S2 / effsamp, "var": S2 / ns - m * m, "kappa": kappa,
            "b": float(sum(8.0 * (P + 2 * K + g) * EPS * k for k in kappa) / effsamp)}


def scaled_panels(Lambda, omega, rho):
    """(Left, Right) of precision_mean_cases.panels with every row divided by sqrt(d_a), d_a = 1 / omega_a -
    LeftG_a . RightG_a - LeftA_a . RightA_a: what k_pc_scale leaves in the factor buffer."""
    ps, Left, Right = mc.panels(Lambda, omega, rho)
    K = Left.shape[1] // 2
    d = ps - np.einsum("ak,ak->a", Left[:, :K], Right[:, :K]) - np.einsum("ak,ak->a", Left[:, K:], Right[:, K:])
    s = 1.0 / np.sqrt(d)
    return Left * s[:, None], Right * s[:, None]


def panel_partial(Lambda, omega, rho):
    """R(s) from the scaled panels: LeftG RightG' + [one shard] LeftA RightA', the lower triangle mirrored and
    the diagonal set to 1, as the device forms it."""
    P = Lambda.shape[0]
    Left, Right = scaled_panels(Lambda, omega, rho)
    p, K = Left.shape[0], Left.shape[1] // 2
    same = (np.arange(p)[:, None] // P) == (np.arange(p)[None, :] // P)
    R = Left[:, :K] @ Right[:, :K].T + np.where(same, Left[:, K:] @ Right[:, K:].T, 0.0)
    R = np.tril(R) + np.tril(R, -1).T
    R[np.diag_indices_from(R)] = 1.0
    return R


def panel_moments(states, rho, effsamp):
    """(PC, PC2) by the scaled-panel restatement."""
    Rs = [panel_partial(st["Lambda"], st["omega"], rho) for st in states]
    return sum(Rs) / effsamp, sum(R * R for R in Rs) / effsamp


def stripe(p):
    """(col0, ncols) of the tests' column stripe: [37, 107) where p allows, else the last half."""
    return (37, 70) if p >= 107 else (p // 2, p - p // 2)


def read_all(smp):
    """Every read-out of an open sampler with partial_corr on (SD only once a sample is saved)."""
    p = smp.P * smp.g
    c0, nc = stripe(p)
    out = {"mean": smp.get_partial_corr("mean"), "m2": smp.get_partial_corr("m2"), "c0": c0, "nc": nc,
           "mean_cols": smp.get_partial_corr_cols("mean", c0, nc), "m2_cols": smp.get_partial_corr_cols("m2", c0, nc),
           "block": smp.sigma_block(), "saved": smp.saved_samples()}
    if out["saved"] > 0:
        out["sd"], out["sd_cols"] = smp.get_partial_corr("sd"), smp.get_partial_corr_cols("sd", c0, nc)
    return out


def run_pc(dcfm, shape, rho=0.5, states=True, case_seed=21, **kw):
    """The injected chain of probe_cases (burnin 1, mcmc 6, thin 2) on `shape` = (n, p, g, K) at rho with the
    partial correlations on, one iteration per run call (`states`: Lambda and omega are read back after every
    saved one; else the chain runs in one call).  Returns read_all's dict plus "states"."""
    n, p, g, K = shape
    c = make_case(n, p, g, K, seed=case_seed, k0=4, rho=rho)
    smp = pc.start(dcfm, c, g, K, partial_corr=True, **kw)
    try:
        sts = []
        if not states:
            smp.run(1, pc.N)
        for it in range(1, pc.N + 1 if states else 0):
            smp.run(it, 1)
            if it in pc.SAVED:
                sts.append(smp.get_state(("Lambda", "omega")))
        out = read_all(smp)
        out["states"] = sts
        return out
    finally:
        smp.close()
