"""The diagonally scaled backward error of the loading draw (helpers.loading_scaled_backward_error): where its
two bars come from, what keeps them from hiding a failure, and the blind spots it closes.  No GPU; reference code
only (oracle/): no figure here comes from the library.

For a row's system Q lam = b + L z (oracle.vectorised.loading_systems) the figures are the measure of
  (a) the vectorised oracle's solve;
  (b) the faithful loop's Lambda (oracle/dc_oracle.py), at the k_paths cases (the replay layouts' 27 iterations
      of the loop are not affordable here and run (a) and (c) only);
  (c) the solve with the factor of Q o (1 + K eps U), U symmetric uniform in [-1, 1], five seeds: a legitimately
      different backward-stable factorisation, since an implementation's own factor is not the oracle's L;
and, as errors a test must catch, of
  (iii) the solve with the factor of Q + 1e-9 ps_j E: a 1e-9 error in the factor's data part;
  (iv)  the solve with one 16 x 16 tile, or one entry, of L times (1 + 1e-9).
They are taken over every k_paths.CASES x 3 iterations of the faithful loop's chain, every flat-start case
(k_paths.flat_case, one iteration) and the four replay layouts (tests/replay_cases.py, 27 iterations of the
vectorised chain).

Bars (tests/helpers.py): SBW_TOL_WELL for rows with cond_2(D Q_j D) <= SBW_COND_WELL = 1e3, SBW_TOL for the others;
each is 8 x the worst of (a)-(c) over its rows, rounded up to one digit (tests/kunit's rule: the device within
8 x of what host arithmetic does).  The tests assert (a)-(c) <= bar / 8 for every row, so a changed case that moves
them fails here first, and test_the_bars_are_eight_times_the_reference holds the constants to 8 ... 12 x the
measurement.  Measured (the REFERENCE_WORST lines this file prints), worst row:

  rows                      cond(DQD)   (a)       (b)       (c)                          (iii), smallest
  CASES, iteration 1        <= 37.1     2.5e-16   3.3e-16   6.3e-15                      2.3e-10
  CASES, iterations 2, 3    <= 4.7e9    2.8e-16   1.1e-15   9.0e-15 (cond <= 1e3),       6.9e-14 (K = 104, iteration 2)
                                                            7.8e-14 (the 752 other rows)
  flat start                <= 290      1.4e-16   2.1e-16   6.2e-15                      1.4e-10
  replay layouts            <= 6.7      3.2e-16   --        4.5e-15                      2.6e-10

so SBW_TOL_WELL = 8e-14 (8 x 9.0e-15 = 7.2e-14; 41 eps measured) and SBW_TOL = 7e-13 (8 x 7.8e-14 = 6.2e-13).  Rows
over cond 1e3 occur only in iterations 2 and 3 of K = 21, 23, 48, 57, 64, 72, 80, 88, 104, 113, 120, 128; every
iteration-1 row, every flat-start row and every replay row is in the well class (asserted).

What keeps the bars from hiding a failure (asserted): SBW_TOL_WELL <= 1 / 100 of the smallest iteration-1 response
to (iii), 2.3e-10, and <= 1 / 10 of the smallest flat-start response to one entry of L times (1 + 1e-9), 1.1e-12
(entry (32, 31) at K = 65).  In the high-cond rows the measure is weak, as it must be: (iii) reads down to 6.9e-14
there, under SBW_TOL; those iterations are held by the other stages' bars.

The blind spots, as tests: at K >= 65, iteration 1, (iii) reads <= 9.9e-15 on the normwise measure (bar 1e-13: it
passes) and >= 2.3e-10 on this one; at the default start for K >= 81 the trailing tile of L times (1 + 1e-9) reads
<= 2.6e-16 on this measure too (tau up to 2e10 makes the trailing tiles of D Q_j D the identity to rounding: no
measure can see what the kernels multiply there); at the flat start the same plant reads >= 1.3e-11 at every wide
K.  The every-tile sweep (test_flat_start_reaches_every_tile): at the flat start one 16 x 16 tile of L times
(1 + 1e-9) moves the worst row to >= 1.3e-11 (tile (7, 6) at K = 113) for every K of k_paths.FLAT_ALL and every
tile of the lower triangle, against 10 x SBW_TOL_WELL = 8e-13: no (K, tile) misses, none needed another n or seed.
"""
import functools

import numpy as np
import pytest

import k_paths as kp
import replay_cases as rc
from helpers import (SBW_COND_WELL, SBW_TOL, SBW_TOL_WELL, LoadingMeasure, loading_backward_error,
                     loading_scaled_backward_error, loading_scaled_bars)
from oracle import dc_oracle as F
from oracle import vectorised as V

EPS = float(np.finfo(np.float64).eps)
BW_TOL = 1e-13                  # the normwise bar of tests/test_gpu_k_paths.py
PLANT = 1e-9
SEEDS = range(5)
LAYOUTS = ["wide64", "wide128", "unfused", "fused"]
TILE = 16


def _mat(lam):
    """g x P x K -> the MATLAB layout P x K x g."""
    return np.moveaxis(lam, 0, 2)


def _systems(start, c, dr, got=None):
    """(E, Q, b, L, z) of the iteration that starts at the oracle state `start`; with `got` (a state after that
    iteration) from its X, Z and eta, as helpers.stagewise_errors forms them."""
    D = V._as_data(c["Yd"])
    st = start.copy()
    V.update_ZX(st, D, c["rho"], dr)
    V.update_eta(st, c["rho"])
    if got is not None:
        for f in ("X", "Z", "eta"):
            getattr(st, f)[...] = getattr(got, f)
    E, _, Q, b, L, z = V.loading_systems(st, D, dr)
    ps = st.ps[:, 0, :].T
    return ps[:, :, None, None] * E[:, None], Q, b, L, z


def _with_factor_of(A, b, z):
    """The draw computed with chol(A) in place of the system's own factor."""
    return V._loading_solve(np.linalg.cholesky(A), b, z)


def _jitter(Q, seed):
    """Q o (1 + K eps U), U symmetric uniform in [-1, 1]."""
    K = Q.shape[-1]
    U = np.triu(np.random.default_rng(seed).uniform(-1.0, 1.0, Q.shape))
    U = U + np.swapaxes(np.triu(U, 1), -1, -2)
    return Q * (1.0 + K * EPS * U)


def _tile_plant(L, ti, tj, b, z):
    """The draw with rows 16 ti ..., columns 16 tj ... of every L_j times (1 + PLANT)."""
    L2 = L.copy()
    L2[..., TILE * ti:TILE * (ti + 1), TILE * tj:TILE * (tj + 1)] *= 1.0 + PLANT
    return V._loading_solve(L2, b, z)


def _entry_plant(L, i, j, b, z):
    L2 = L.copy()
    L2[..., i, j] *= 1.0 + PLANT
    return V._loading_solve(L2, b, z)


def _figures(psE, Q, b, L, z, lam_b=None):
    """The reference figures of one iteration's systems (floats; `lam_b` the faithful loop's Lambda, g x P x K)."""
    sm = LoadingMeasure(Q, b, L, z)
    cond = sm.cond

    def m(lam):
        return sm(_mat(lam))
    a = m(V._loading_solve(L, b, z))
    fb = m(lam_b) if lam_b is not None else np.zeros_like(a)
    fc = np.max([m(_with_factor_of(_jitter(Q, s), b, z)) for s in SEEDS], axis=0)
    lam3 = _with_factor_of(Q + PLANT * psE, b, z)
    well = cond <= SBW_COND_WELL
    ref = np.maximum(np.maximum(a, fb), fc)
    return dict(measure=sm, cond_max=float(cond.max()), n_ill=int((~well).sum()), n_rows=int(well.size),
                a=float(a.max()), b=float(fb.max()), c=float(fc.max()),
                ref_well=float(ref[well].max()) if well.any() else 0.0, ref_all=float(ref.max()),
                ref_over_bar=float((ref / loading_scaled_bars(cond)).max()),
                iii=float(m(lam3).max()), iii_old=loading_backward_error(_mat(lam3), Q, b, L, z),
                iii_over_bar=float((m(lam3) / loading_scaled_bars(cond)).max()))


def _nb(K):
    return (K + TILE - 1) // TILE


def _trailing_tile(K):
    """The last off-diagonal tile of the factor (the diagonal one where the factor is a single tile)."""
    nb = _nb(K)
    return nb - 1, max(nb - 2, 0)


@functools.lru_cache(maxsize=None)
def default_figures(K):
    """One dict per iteration of case K's faithful-loop chain; iteration 1 also with the trailing tile planted."""
    c = kp.case(K)
    ref = c["st"].copy()
    out = []
    for it in range(1, kp.N_ITER + 1):
        start = ref.copy()
        dr = c["src"].iteration(it)
        F.gibbs_iteration(ref, c["Yd"], c["rho"], c["hyper"], dr)
        psE, Q, b, L, z = _systems(start, c, dr, ref)
        r = _figures(psE, Q, b, L, z, np.moveaxis(ref.Lambda, 2, 0))
        if it == 1:
            lam = _mat(_tile_plant(L, *_trailing_tile(K), b, z))
            r["trail"] = float(r["measure"](lam).max())
            r["trail_old"] = loading_backward_error(lam, Q, b, L, z)
        del r["measure"]
        out.append(r)
    return out


@functools.lru_cache(maxsize=None)
def flat_figures(K):
    """The flat-start case's one iteration: the reference figures, cond(Q_j), max|X|, the response of every tile of
    the lower triangle and of two single entries to the 1e-9 plant."""
    c = kp.flat_case(K)
    ref = c["st"].copy()
    dr = c["src"].iteration(1)
    F.gibbs_iteration(ref, c["Yd"], c["rho"], c["hyper"], dr)
    psE, Q, b, L, z = _systems(c["st"], c, dr, ref)
    r = _figures(psE, Q, b, L, z, np.moveaxis(ref.Lambda, 2, 0))

    sm = r.pop("measure")

    def m(lam):
        return float(sm(_mat(lam)).max())
    r["condQ_max"] = float(np.linalg.cond(Q).max())
    r["xmax"] = float(np.abs(ref.X).max())
    r["tiles"] = {(ti, tj): m(_tile_plant(L, ti, tj, b, z)) for ti in range(_nb(K)) for tj in range(ti + 1)}
    r["trail"] = r["tiles"][_trailing_tile(K)]
    r["entries"] = {ij: m(_entry_plant(L, *ij, b, z)) for ij in ((K // 2, K // 2 - 1), (K - 1, K - 2))}
    return r


@functools.lru_cache(maxsize=None)
def replay_figures(layout):
    """One dict per iteration of the layout's 27-iteration chain (vectorised oracle, the replay tests' draws)."""
    from oracle import philox_ref as R
    c = rc.case(layout)
    src = R.PhiloxSource(rc.CHAIN_SEED, c["n"], c["p"], c["g"], c["K"], c["hyper"])
    D = V._as_data(c["Yd"])
    st = c["st"].copy()
    out = []
    for it in range(1, rc.N + 1):
        start = st.copy()
        dr = src.iteration(it)
        V.gibbs_iteration(st, D, c["rho"], c["hyper"], dr)
        out.append(_figures(*_systems(start, c, dr)))
        del out[-1]["measure"]
    return out


def _all_default():
    return [(f"K = {K} iteration {it}", r) for K in kp.CASES for it, r in enumerate(default_figures(K), 1)]


def _all_flat():
    return [(f"flat K = {K}", flat_figures(K)) for K in kp.FLAT_ALL]


def _all_replay():
    return [(f"{lay} iteration {it}", r) for lay in LAYOUTS for it, r in enumerate(replay_figures(lay), 1)]


def test_the_measure_on_a_known_system():
    """2 x 2 by hand: Q = [[4, 2], [2, 1e20 + 1]], L = [[2, 0], [1, 1e10]]; D Q D has unit diagonal and off-diagonal
    1e-10, so cond = 1 to rounding; an exact draw measures 0; an error of relative size t in lam_0 alone reads
    ~ t / 3 on the scaled measure and ~ t 4e-20 on the normwise one."""
    Q = np.array([[4.0, 2.0], [2.0, 1e20 + 1.0]])[None, None]
    L = np.linalg.cholesky(Q)
    b = np.array([1.0, 1.0])[None, None]
    z = np.zeros((1, 1, 2))
    lam = V._loading_solve(L, b, z)
    sbw, cond = loading_scaled_backward_error(_mat(lam), Q, b, L, z)
    assert sbw.shape == cond.shape == (1, 1)
    assert sbw[0, 0] <= 2 * EPS and abs(cond[0, 0] - 1.0) <= 1e-9
    t = 1e-6
    off = lam * np.array([1.0 + t, 1.0])
    sbw, Dr = LoadingMeasure(Q, b, L, z)(_mat(off), residual=True)
    assert Dr.shape == (1, 1, 2)
    # r = Q (off - lam) = t lam_0 (4, 2); D = (1/2, 1e-10); lam_0 = 1/4 to 1e-20:  || D r || = t / 2;
    # the denominator: || D Q D || = 1, || D^-1 lam || = 1/2 (lam_1 ~ 5e-21), || D b || = 1/2, z = 0
    assert abs(sbw[0, 0] / (t / 2.0) - 1.0) <= 1e-6
    assert abs(Dr[0, 0, 0] / (t / 2.0) - 1.0) <= 1e-6 and abs(Dr[0, 0, 1]) <= 1e-15
    assert loading_backward_error(_mat(off), Q, b, L, z) <= 1e-25
    bars = loading_scaled_bars(np.array([1.0, SBW_COND_WELL, 1.001 * SBW_COND_WELL, np.inf]))
    assert list(bars) == [SBW_TOL_WELL, SBW_TOL_WELL, SBW_TOL, SBW_TOL] and SBW_TOL_WELL < SBW_TOL


@pytest.mark.parametrize("K", kp.CASES, ids=kp.case_id)
def test_reference_sits_under_the_bars(K):
    for it, r in enumerate(default_figures(K), 1):
        print("SBW_REFERENCE", kp.case_id(K), f"iter {it}", {k: (f"{v:.2e}" if isinstance(v, float) else v)
                                                               for k, v in sorted(r.items())})
        assert r["ref_over_bar"] <= 1.0 / 8.0, \
            f"K = {K} iteration {it}: the reference's own scaled error is {r['ref_over_bar']:.3g} of its row's bar"
        if it == 1:
            assert r["n_ill"] == 0, f"K = {K}: iteration 1 has {r['n_ill']} rows with cond(DQD) > {SBW_COND_WELL:g}"


@pytest.mark.parametrize("K", kp.FLAT_ALL, ids=kp.case_id)
def test_flat_start_reference_sits_under_the_bars(K):
    r = flat_figures(K)
    print("SBW_REFERENCE_FLAT", kp.case_id(K), {k: (f"{v:.2e}" if isinstance(v, float) else v)
                                                for k, v in sorted(r.items()) if not isinstance(v, dict)})
    assert r["n_ill"] == 0, f"flat K = {K}: {r['n_ill']} rows with cond(DQD) > {SBW_COND_WELL:g}"
    assert r["ref_well"] <= SBW_TOL_WELL / 8.0, f"flat K = {K}: the reference's own scaled error {r['ref_well']:.3e}"


@pytest.mark.parametrize("layout", LAYOUTS)
def test_replay_reference_sits_under_the_bars(layout):
    rs = replay_figures(layout)
    assert len(rs) == rc.N
    print("SBW_REFERENCE_REPLAY", layout, {k: f"{max(r[k] for r in rs):.2e}" for k in ("cond_max", "a", "c")},
          f"iii min {min(r['iii'] for r in rs):.2e}")
    for it, r in enumerate(rs, 1):
        assert r["n_ill"] == 0, f"{layout} iteration {it}: {r['n_ill']} rows with cond(DQD) > {SBW_COND_WELL:g}"
        assert r["ref_well"] <= SBW_TOL_WELL / 8.0, f"{layout} iteration {it}: reference at {r['ref_well']:.3e}"
        assert r["iii"] >= 100.0 * SBW_TOL_WELL, f"{layout} iteration {it}: a 1e-9 factor error reads {r['iii']:.3e}"


def test_the_bars_are_eight_times_the_reference():
    """The two constants against the measurement they come from, and the conditions that keep them from hiding a
    failure."""
    everything = _all_default() + _all_flat() + _all_replay()
    ref_well = max(r["ref_well"] for _, r in everything)
    ref_all = max(r["ref_all"] for _, r in everything)
    n_ill = sum(r["n_ill"] for _, r in everything)
    n_rows = sum(r["n_rows"] for _, r in everything)
    for name, sel in (("CASES iteration 1", [r for K in kp.CASES for r in default_figures(K)[:1]]),
                      ("CASES iterations 2, 3", [r for K in kp.CASES for r in default_figures(K)[1:]]),
                      ("flat start", [r for _, r in _all_flat()]), ("replay", [r for _, r in _all_replay()])):
        print("REFERENCE_WORST", name, {k: f"{max(r[k] for r in sel):.2e}" for k in
                                        ("cond_max", "a", "b", "c", "ref_well", "ref_all")},
              f"iii min {min(r['iii'] for r in sel):.2e}", "rows over cond 1e3:", sum(r["n_ill"] for r in sel))
    print(f"REFERENCE_WORST all: well {ref_well:.3e} ({ref_well / EPS:.1f} eps), overall {ref_all:.3e} "
          f"({ref_all / EPS:.1f} eps), {n_ill} of {n_rows} rows over cond {SBW_COND_WELL:g}")
    assert n_ill > 0, "no case reaches the high-cond class: SBW_TOL is not exercised"
    # 8 x the worst, rounded up to one digit: neither under it nor above 12 x
    assert 8.0 * ref_well <= SBW_TOL_WELL <= 12.0 * ref_well, f"SBW_TOL_WELL {SBW_TOL_WELL:g} vs 8 x {ref_well:.3e}"
    assert 8.0 * ref_all <= SBW_TOL <= 12.0 * ref_all, f"SBW_TOL {SBW_TOL:g} vs 8 x {ref_all:.3e}"
    iii1 = min(default_figures(K)[0]["iii"] for K in kp.CASES)
    entry = min(min(flat_figures(K)["entries"].values()) for K in kp.FLAT_ALL)
    print(f"REFERENCE_WORST responses: (iii) at iteration 1 >= {iii1:.3e}, single entries at the flat start >= {entry:.3e}")
    assert SBW_TOL_WELL <= iii1 / 100.0
    assert SBW_TOL_WELL <= entry / 10.0


# ---- the blind spots, stated as tests ---------------------------------------------------------------------
@pytest.mark.parametrize("K", [K for K in kp.CASES if K >= 65], ids=kp.case_id)
def test_factor_error_passes_the_old_bar_and_fails_the_new(K):
    r = default_figures(K)[0]
    assert r["iii_old"] <= BW_TOL, f"K = {K}: the normwise measure reads {r['iii_old']:.3e}"
    assert r["iii"] >= 100.0 * SBW_TOL_WELL, f"K = {K}: the scaled measure reads {r['iii']:.3e}"


@pytest.mark.parametrize("K", [K for K in kp.CASES if K >= 81], ids=kp.case_id)
def test_default_start_does_not_see_the_trailing_tile(K):
    """Not the measure's fault: at the default start the trailing tiles of D Q_j D are the identity to rounding."""
    r = default_figures(K)[0]
    assert r["trail"] <= SBW_TOL_WELL and r["trail_old"] <= BW_TOL, f"K = {K}: {r['trail']:.3e}, {r['trail_old']:.3e}"


@pytest.mark.parametrize("K", kp.FLAT_ALL, ids=kp.case_id)
def test_flat_start_reaches_every_tile(K):
    r = flat_figures(K)
    worst = min((v, t) for t, v in r["tiles"].items())
    print("SBW_TILES", kp.case_id(K), f"{len(r['tiles'])} tiles, lowest response {worst[0]:.2e} at tile {worst[1]},",
          f"trailing tile {r['trail']:.2e}, entries", {ij: f"{v:.2e}" for ij, v in r["entries"].items()})
    assert len(r["tiles"]) == _nb(K) * (_nb(K) + 1) // 2
    for t, v in r["tiles"].items():
        assert v > 10.0 * SBW_TOL_WELL, f"flat K = {K}: tile {t} of L times (1 + 1e-9) reads {v:.3e}"
