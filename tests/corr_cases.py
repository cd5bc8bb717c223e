"""Shared setup of the correlation tests (test_corr_host.py, test_gpu_corr.py): the dense NumPy reference of the two
moments of the per-sample correlation matrix R(s) = D(s)^-1/2 Sigma(s) D(s)^-1/2 (Sigma(s) the oracle's, D(s) its
diagonal) and of the communalities h_a(s) = |Lambda_a(s)|^2 / Sigma(s)_aa; the NumPy restatement of csrc/corr.hip
(the scale applied to the panels before the product, tile by tile); the entrywise bound; and the short injected
chain of probe_cases with DCFM_FLAG_CORR set.

The bound (derived, not measured).  No inversion is involved and |R| <= 1, so no condition number enters.  Per
sample the scaled dot product and the two scales lose at most about (2K + 8) eps on an entry (Cauchy-Schwarz:
sum_k |l_ak l_bk| s_a s_b <= 1), the reference about (K + 4) eps, together below 4 (K + 4) eps; summing `saved`
terms adds saved eps.  With the 1/effsamp scaling

    b = (saved / effsamp) (4 (K + 4) + saved) eps

bounds max|C - ref|; 2 b the second moment (|t^2 - t_ref^2| <= 2 |t| err, |t| <= 1); 4 r b the variance, r =
effsamp / saved (var = r C2 - (r C)^2: r 2b + 2 r b).  0 <= h <= 1 is a ratio of the same sums: the same bars."""
import numpy as np

import probe_cases as pc
from helpers import make_case

EPS = pc.EPS
TILE = 128

# ((n, p, g, K), rho): what each shape covers on the device
SWEEP = [
    ((30, 48, 4, 5), 0.5),         # K odd, four shards in one partial tile
    ((30, 36, 3, 1), 0.5),         # K = 1
    ((24, 120, 20, 2), 0.5),       # P = 6, twenty shards in a tile: the per-pair coefficient
    ((24, 130, 2, 4), 0.5),        # P = 65: a shard edge off the tile edge
    ((37, 300, 3, 7), 0.5),        # mixed tiles
    ((37, 300, 3, 7), 0.0),
    ((37, 300, 3, 7), 1.0),
    ((64, 384, 3, 30), 0.5),       # P = 128: pure cross and pure same-shard tiles
    ((50, 128, 2, 32), 0.5),       # K = 32
    ((40, 99, 3, 33), 0.5),        # wide layout
    ((32, 1152, 9, 3), 0.5),       # crosses a supertile
    ((120, 200, 2, 100), 0.5),     # K = 100
    ((140, 256, 2, 128), 0.5),     # K = 128
]


def bound(K, saved, effsamp):
    """b of the module docstring."""
    return (saved / effsamp) * (4 * (K + 4) + saved) * EPS


def rows(Lambda, omega):
    """(L p x K, w p) in Sigmaout's row order from Lambda P x K x g and omega P x g: row m P + j is shard m's j."""
    Lambda, omega = np.asarray(Lambda, dtype=np.float64), np.asarray(omega, dtype=np.float64)
    P, K, g = Lambda.shape
    return np.ascontiguousarray(Lambda.transpose(2, 0, 1).reshape(P * g, K)), omega.T.reshape(P * g)


def sample_corr(Lambda, omega, rho):
    """R(s) from the oracle's dense Sigma(s) divided by sqrt(diag x diag), the diagonal set to 1."""
    Sig = pc.sample_sigma(Lambda, omega, rho)
    v = Sig.diagonal().copy()
    R = Sig / np.sqrt(np.outer(v, v))
    R[np.diag_indices_from(R)] = 1.0
    return R


def sample_communality(Lambda, omega):
    """h(s) from Lambda and omega directly."""
    L, w = rows(Lambda, omega)
    ss = np.sum(L * L, axis=1)
    return ss / (ss + w)


def dense_moments(states, rho, effsamp):
    """{"C": (1/effsamp) sum_s R(s), "C2": the same sum of R(s)^2, "var": the population variance of R(s) over the
    saved samples, "H", "H2", "hvar": the same for the communalities, "b": bound(K, saved, effsamp)}."""
    P, K, g = states[0]["Lambda"].shape
    p, ns = P * g, len(states)
    S1, S2, h1, h2 = np.zeros((p, p)), np.zeros((p, p)), np.zeros(p), np.zeros(p)
    for st in states:
        R, h = sample_corr(st["Lambda"], st["omega"], rho), sample_communality(st["Lambda"], st["omega"])
        S1 += R
        S2 += R * R
        h1 += h
        h2 += h * h
    m, hm = S1 / ns, h1 / ns
    return {"C": S1 / effsamp, "C2": S2 / effsamp, "var": S2 / ns - m * m, "H": h1 / effsamp, "H2": h2 / effsamp,
            "hvar": h2 / ns - hm * hm, "b": bound(K, ns, effsamp)}


def device_sample(Lambda, omega, rho):
    """(R(s), h(s), s) as csrc/corr.hip forms them: v = |L_a|^2 + omega_a, s = 1 / sqrt(v), h = |L_a|^2 / v; per
    128 x 128 lower tile the row panel times s_a (times rho on a tile whose rows' first shard is past its columns'
    last), the column panel times s_b, then the product, times the per-pair coefficient on the other tiles; the
    lower triangle mirrored, the diagonal 1."""
    L, w = rows(Lambda, omega)
    P = np.asarray(Lambda).shape[0]
    p = L.shape[0]
    ss = np.sum(L * L, axis=1)
    v = ss + w
    s = 1.0 / np.sqrt(v)
    shard = np.arange(p) // P
    R = np.zeros((p, p))
    for r0 in range(0, p, TILE):
        r1 = min(p, r0 + TILE)
        for c0 in range(0, r0 + 1, TILE):
            c1 = min(p, c0 + TILE)
            cross = shard[r0] > shard[c1 - 1]
            A = L[r0:r1] * ((rho if cross else 1.0) * s[r0:r1])[:, None]
            Bm = L[c0:c1] * s[c0:c1, None]
            G = A @ Bm.T
            if not cross:
                G = np.where(shard[r0:r1, None] == shard[None, c0:c1], 1.0, rho) * G
            R[r0:r1, c0:c1] = G
    R = np.tril(R) + np.tril(R, -1).T
    R[np.diag_indices_from(R)] = 1.0
    return R, ss / v, s


def device_moments(states, rho, effsamp):
    """{"C", "C2", "H", "H2"} by the restatement, accumulated as the device does within a flush."""
    p = states[0]["Lambda"].shape[0] * states[0]["Lambda"].shape[2]
    S1, S2, h1, h2 = np.zeros((p, p)), np.zeros((p, p)), np.zeros(p), np.zeros(p)
    for st in states:
        R, h, _ = device_sample(st["Lambda"], st["omega"], rho)
        S1 += R
        S2 += R * R
        h1 += h / effsamp
        h2 += h * h / effsamp
    return {"C": S1 / effsamp, "C2": S2 / effsamp, "H": h1, "H2": h2}


def stripe(p):
    """(col0, ncols) of the tests' column stripe: [37, 107) where p allows, else the last half."""
    return (37, 70) if p >= 107 else (p // 2, p - p // 2)


def read_all(smp):
    """Every read-out of an open sampler with corr on (the SDs only once a sample is saved)."""
    p = smp.P * smp.g
    c0, nc = stripe(p)
    out = {"mean": smp.get_corr("mean"), "m2": smp.get_corr("m2"), "c0": c0, "nc": nc,
           "mean_cols": smp.get_corr_cols("mean", c0, nc), "m2_cols": smp.get_corr_cols("m2", c0, nc),
           "h": smp.get_communality("mean"), "h2": smp.get_communality("m2"),
           "block": smp.sigma_block(), "saved": smp.saved_samples()}
    if out["saved"] > 0:
        out["sd"], out["sd_cols"] = smp.get_corr("sd"), smp.get_corr_cols("sd", c0, nc)
        out["hsd"] = smp.get_communality("sd")
    return out


def run_corr(dcfm, shape, rho=0.5, states=True, case_seed=21, **kw):
    """The injected chain of probe_cases (burnin 1, mcmc 6, thin 2) on `shape` = (n, p, g, K) at rho with the
    correlations on, one iteration per run call (`states`: Lambda and omega are read back after every saved one;
    else the chain runs in one call).  Returns read_all's dict plus "states"."""
    n, p, g, K = shape
    c = make_case(n, p, g, K, seed=case_seed, k0=4, rho=rho)
    smp = pc.start(dcfm, c, g, K, corr=True, **kw)
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
