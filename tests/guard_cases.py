r"""Planted high-cancellation rows for the guard of the SS identity (csrc/resid.h, ss_identity_reject), and a
float64 restatement of the guard's decision.  Plain NumPy, no GPU; tests/test_guard_cases.py checks the
construction on the reference alone, tests/test_gpu_guard.py runs the cases on the device.

The construction.  From a start state with Lambda = 0 the first iteration's eta does not depend on Yd (W = 0
and A = 0, so Z = eps_z and X = eps_x / sqrt(g)).  So eta_1 is computed from the injected draws first and a
column of Yd is built around it: for a planted row (m, j) with scale s

    Yd[:, j, m] = s * eta_1[:, :, m] @ l + noise,            l ~ N(0, I_K), noise ~ N(0, I_n),

and in the start state ps[j, m] = omega[j, m] = 1, Plam[j, :, m] = 1e-12 (iteration 1 uses the caller's Plam:
no shrinkage bias).  The loading draw then fits lambda_j ~ s l, the residual is the noise (SS_j ~ n, far above
bs = 0.3, so ps_j really depends on SS_j), and the identity SS_j = yy_j - 2 lambda_j.C_j + lambda_j E lambda_j'
sums terms of order s^2 n |l|^2: kappa_j ~ c s^2.  A zero column (yy_j = 0) is planted by zeroing Yd[:, j, m].

Two-iteration cases set the start state again before the second iteration (same handle, same data) and do not
continue the chain: a loading row of order s makes the reference's next Z draw (dc:104, R' \ (R \ b) with an
upper R) an excursion.  Measured on the oracle from a continued chain at (40, 21, 2, 12): s = 30 gives |eta| up to
4e6 and every one of the 42 rows 'reject' at iteration 2, s >= 100 a Gram matrix E with eigenvalues -5.6e10 ...
4.9e26 whose Cholesky factorisation fails; the same at (45, 545, 1, 33).  From the start state eta_2 is as
independent of Yd as eta_1, so a row is planted around the eta of the iteration it is meant to cancel at
(m, j, s, it) and is plain noise at the other: the rows rejected at iteration 1 are accepted at iteration 2 and
the other way round, which is what shows a stale flag or a flag cleared too early.

guard_ratio restates num_j / SS_j of ss_identity_reject from a state (eta and Lambda taken as given),
classify() sorts a row by it with a factor 2 either side of KAPPA_MAX: the restatement and the device differ by
rounding of about (n + K) eps relative near the threshold, so a row outside the band has the same decision on
both; a row inside it ("grey") gets accuracy assertions only.
"""
import functools

import numpy as np

KAPPA_MAX = 1e3                 # csrc/resid.h, KAPPA_IDENTITY_MAX
BAND = 2.0                      # classify(): reject above BAND * KAPPA_MAX, accept below KAPPA_MAX / BAND
PLANT_PLAM = 1e-12
SEED = 5

# name: shape (n, P, g, K), plants ((shard m, row j, scale s, iteration it), ...), zero columns ((m, j), ...),
# iterations.  Every iteration starts from the case's start state (Lambda = 0, set again on the same handle) and
# is saved (burn-in 0, thin 1); a row planted around eta_it cancels at iteration it alone (at the other one its
# column is noise against that iteration's eta: SS_j ~ yy_j).  Narrow (K <= 32): a wave of k_lambda holds 8
# loading rows; wide: k_resid_flagged works on tiles of 32 rows, at most 16 blocks per shard.
CASES = {
    # wave 0 of shard 0 (row 3), the last valid row of its partial wave (row 20: P = 21), wave 1 of shard 1 with
    # an identity SS that is garbage (s = 1e9), a zero column in wave 0 of shard 1; wave 1 of shard 0 and wave 2
    # of shard 1 stay clean
    "narrowA": dict(shape=(40, 21, 2, 7), plants=((0, 3, 1e3, 1), (0, 20, 1e6, 1), (1, 8, 1e9, 1)),
                    zero_cols=((1, 5),), n_iter=1),
    # the same plants under k_lambda<30> (four row blocks per lane, rows 30 and 31 padding)
    "narrowB": dict(shape=(40, 21, 2, 30), plants=((0, 3, 1e3, 1), (0, 20, 1e6, 1), (1, 8, 1e9, 1)),
                    zero_cols=((1, 5),), n_iter=1),
    # k_lambda<16>, two saved iterations, s = 1e3 only (Sigmaout still sees an omega beside lambda lambda'): the
    # switched wave is shard 1's wave 1 at iteration 1 and shard 0's wave 0 at iteration 2
    "narrowC": dict(shape=(40, 21, 2, 12), plants=((1, 10, 1e3, 1), (0, 2, 1e3, 2)), zero_cols=(), n_iter=2),
    # KW = 64: a plant in tile 0 and one in the partial tile 1 of shard 0 (rows 32 .. 36), none in shard 1.  n = 65:
    # at n = 45 an unplanted row reaches a ratio of 864 (n barely above K: the regression nearly interpolates),
    # at n = 65 the largest is 102
    "wideD": dict(shape=(65, 37, 2, 40), plants=((0, 5, 1e3, 1), (0, 36, 1e6, 1)), zero_cols=(), n_iter=1),
    # KW = 128: one plant, in shard 1's one-row tile
    "wideE": dict(shape=(100, 33, 2, 70), plants=((1, 32, 1e6, 1),), zero_cols=(), n_iter=1),
    # PP = 576: 18 tiles over 16 blocks.  Iteration 1: tiles 0 and 16 (block 0 runs both), tile 17 (block 1 skips
    # its first tile and runs its second: row 544 is tile 17's one valid row), tile 2.  Iteration 2: those four
    # tiles are clean again (a flag left set would redo them) while tile 1 (block 1 runs its first tile and skips
    # its second) and tile 5 reject.  Two saved iterations
    "wideF": dict(shape=(45, 545, 1, 33),
                  plants=((0, 7, 1e3, 1), (0, 521, 1e3, 1), (0, 544, 3e2, 1), (0, 95, 1e2, 1),
                          (0, 40, 1e3, 2), (0, 170, 3e2, 2)), zero_cols=(), n_iter=2),
}
NARROW_ROWS, WIDE_ROWS, WIDE_BLOCKS = 8, 32, 16


def is_wide(name):
    return CASES[name]["shape"][3] > 32


def group_rows(name):
    """Rows per unit of the fallback: a wave's 8 (K <= 32), a tile's 32 (K > 32)."""
    return WIDE_ROWS if is_wide(name) else NARROW_ROWS


def planted_rows(name, it):
    """[(m, j)] of every row planted to reject at iteration `it`: the rows scaled around eta_it and the zero
    columns."""
    c = CASES[name]
    return [(m, j) for m, j, _, t in c["plants"] if t == it] + [tuple(z) for z in c["zero_cols"]]


def eta_first(st, Yd, rho, draws):
    """eta after iteration 1's Z and X draws from the start state `st` (oracle.vectorised)."""
    from oracle import vectorised as V
    t = st.copy()
    V.update_ZX(t, V.Data(Yd), rho, draws)
    V.update_eta(t, rho)
    return t.eta


def plant(case, plants, zero_cols=()):
    """The construction of the module docstring on a helpers.make_case dict: returns a copy of `case` whose Yd and
    start state st (Lambda = 0) carry the planted rows (m, j, s, it): the column is built around eta_it, the eta
    of iteration it's draws from that start state; the draw source is the case's own."""
    st = case["st"].copy()
    assert not np.any(st.Lambda), "the construction needs a start state with Lambda = 0"
    Yd = np.array(case["Yd"], dtype=np.float64, order="F")
    n, P, g = Yd.shape
    K = st.Lambda.shape[1]
    eta = {it: eta_first(st, Yd, case["rho"], case["src"].iteration(it)) for it in sorted({p[3] for p in plants})}
    for m, j, s, it in plants:
        r = np.random.Generator(np.random.PCG64(np.random.SeedSequence([SEED, 77, m, j])))
        l, noise = r.standard_normal(K), r.standard_normal(n)
        Yd[:, j, m] = s * (eta[it][:, :, m] @ l) + noise
        st.ps[j, 0, m] = 1.0
        st.omega[j, m] = 1.0
        st.Plam[j, :, m] = PLANT_PLAM
    for m, j in zero_cols:
        Yd[:, j, m] = 0.0
    out = dict(case)
    out.update(Yd=Yd, st=st, eta=eta)
    return out


@functools.lru_cache(maxsize=None)
def planted_case(name):
    """CASES[name] built once (read only)."""
    from helpers import make_case
    c = CASES[name]
    n, P, g, K = c["shape"]
    base = make_case(n, P * g, g, K, seed=SEED)
    assert (base["n"], base["P"]) == (n, P), "preprocessing dropped a column"
    out = plant(base, c["plants"], c["zero_cols"])
    out["Yd"].setflags(write=False)
    return out


def guard_parts(start, got, Yd, draws, wide):
    """The sums ss_identity_reject is given for every row, in float64 NumPy, as the loading-row kernels form
    them (csrc/lambda.h, the epilogue of k_lambda_w in csrc/kernels_wide.hip).  `start` is the oracle state at
    the iteration's start (ps and Plam of the previous iteration), `got` maps "eta" and "Lambda" to the state
    after it (MATLAB layout), both taken as given.  Every entry g x P:
      yy, ww = |w|^2 (w = v + z, v = L_Q^{-1} b), wv = w.v, px = sum_r Plam_jr lambda_jr^2, lc = lambda_j.C_j,
      cs = max(1, max_k Q_kk / L_kk^2), sabs = sum_k |lambda_jk| sqrt(E_kk),
      SS: the identity as the kernel sums it (narrow: yy + (ww - px - 2 wv) / ps; wide: yy + (ww - px) / ps -
          2 lambda.C),
      mag: (1 + cs) ww / ps + px / ps + 2 sum_r |w_r v_r| / ps (narrow), ... + 2 sum_r |lambda_jr C_jr| (wide),
      num: max((1.01 (sqrt(yy) + sabs))^2, 1.01 (yy + mag))."""
    from oracle import vectorised as V
    D = V._as_data(Yd)
    st = start.copy()
    st.eta[...] = np.asarray(got["eta"], dtype=np.float64).reshape(st.eta.shape)
    E, C, Q, b, L, z = V.loading_systems(st, D, draws)
    lam = np.ascontiguousarray(np.moveaxis(np.asarray(got["Lambda"], dtype=np.float64), 2, 0))     # g x P x K
    ps = st.ps[:, 0, :].T                                                                         # g x P
    plam = np.moveaxis(st.Plam, 2, 0)                                                             # g x P x K
    v = np.linalg.solve(L, b[..., None])[..., 0]
    w = v + z
    ww = np.einsum("mjk,mjk->mj", w, w)
    wv = np.einsum("mjk,mjk->mj", w, v)
    px = np.einsum("mjk,mjk->mj", plam, lam * lam)
    lc = np.einsum("mjk,mjk->mj", lam, C)
    qd = np.diagonal(Q, axis1=-2, axis2=-1)
    ld = np.diagonal(L, axis1=-2, axis2=-1)
    cs = np.maximum(1.0, np.max(qd / (ld * ld), axis=-1))
    ed = np.sqrt(np.maximum(np.diagonal(E, axis1=-2, axis2=-1), 0.0))                             # g x K
    sabs = np.einsum("mjk,mk->mj", np.abs(lam), ed)
    yy = D.yy
    if wide:
        SS = yy + ((ww - px) / ps - 2.0 * lc)
        last = 2.0 * np.einsum("mjk,mjk->mj", np.abs(lam), np.abs(C))
    else:
        SS = yy + (ww - px - 2.0 * wv) / ps
        last = 2.0 * np.sum(np.abs(w * v), axis=-1) / ps
    mag = ((1.0 + cs) * ww + px) / ps + last
    rt = 1.01 * (np.sqrt(yy) + sabs)
    num = np.maximum(rt * rt, 1.01 * (yy + mag))
    return dict(yy=yy, ww=ww, wv=wv, px=px, lc=lc, cs=cs, sabs=sabs, SS=SS, mag=mag, num=num, ps=ps, E=E, C=C, Q=Q,
                lam=lam)


def guard_ratio(start, got, Yd, draws, wide):
    """num_j / SS_j of ss_identity_reject per row (g x P), the number the device compares with KAPPA_MAX;
    infinity where the guard rejects whatever the ratio: SS_j <= 0 or not finite, yy_j <= 0."""
    p = guard_parts(start, got, Yd, draws, wide)
    SS, yy = p["SS"], p["yy"]
    ok = np.isfinite(SS) & (SS > 0.0) & (yy > 0.0)
    return np.where(ok, p["num"] / np.where(ok, SS, 1.0), np.inf)


def classify(ratio):
    """'reject' above BAND * KAPPA_MAX, 'accept' below KAPPA_MAX / BAND, 'grey' between (and for NaN)."""
    ratio = np.asarray(ratio, dtype=np.float64)
    out = np.full(ratio.shape, "grey", dtype="<U6")
    out[ratio > BAND * KAPPA_MAX] = "reject"
    out[ratio < KAPPA_MAX / BAND] = "accept"
    return out


def summary(ratio, cls):
    """The figures of one case-iteration's log line: the class counts, the largest ratio of an accepted row and
    the smallest of a rejected one."""
    acc, rej = ratio[cls == "accept"], ratio[cls == "reject"]
    return dict(n_accept=int(acc.size), n_grey=int(np.sum(cls == "grey")), n_reject=int(rej.size),
                max_accept_ratio=float(acc.max()) if acc.size else 0.0,
                min_reject_ratio=float(rej.min()) if rej.size else float("inf"))
