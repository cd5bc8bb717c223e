"""CPU tests of the correlation moments (DCFM_FLAG_CORR, dcfm_get_corr[_cols], dcfm_get_communality): the NumPy
restatement of csrc/corr.hip against the dense reference (the oracle's Sigma(s) divided by sqrt(diag x diag)) on the
oracle's own chain, for every shape of the GPU sweep -- the check that the reference alone stays within the bars
of corr_cases; h = 1 - omega s^2 and |R| <= 1; driver.unpermute_corr / unpermute_communality; diagnostics.correlation;
the header and the ctypes binding agree on the new flag and symbols; a null handle is refused without a GPU."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import corr_cases as cc
import precision_cases as qc
import probe_cases as pc
from helpers import rel_err

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "dcfm.h"


@pytest.mark.parametrize("shape,rho", cc.SWEEP)
def test_restatement_matches_the_dense_reference(shape, rho):
    """Bars: entrywise b on both means and 2 b on both second moments, normwise the project's 1e-10."""
    states = qc.oracle_states(shape, rho=rho)
    saved = len(states)
    assert saved == len(pc.SAVED)
    ref = cc.dense_moments(states, rho, pc.EFFSAMP)
    got = cc.device_moments(states, rho, pc.EFFSAMP)
    b = ref["b"]
    assert b == cc.bound(shape[3], saved, pc.EFFSAMP)
    e = {f: float(np.max(np.abs(got[f] - ref[f]))) for f in ("C", "C2", "H", "H2")}
    print(f"{shape} rho={rho}: b {b:.3e}, max|C - ref| {e['C']:.3e}, max|C2 - ref| {e['C2']:.3e}, max|H - ref| "
          f"{e['H']:.3e}, max|H2 - ref| {e['H2']:.3e}, rel_err {rel_err(got['C'], ref['C']):.3e} / "
          f"{rel_err(got['C2'], ref['C2']):.3e}")
    assert e["C"] <= b and e["H"] <= b
    assert e["C2"] <= 2 * b and e["H2"] <= 2 * b
    for f in ("C", "C2", "H", "H2"):
        assert rel_err(got[f], ref[f]) < 1e-10, f
    for M in (got["C"], got["C2"], ref["C"], ref["C2"]):
        assert np.array_equal(M, M.T)
        assert np.array_equal(M.diagonal(), np.full(M.shape[0], saved / pc.EFFSAMP))
        assert np.all(np.abs(M) <= saved / pc.EFFSAMP)
    rs = pc.EFFSAMP / saved
    assert np.all(ref["var"] >= -4 * rs * b) and not ref["var"].diagonal().any()
    assert np.all(ref["hvar"] >= -4 * rs * b)


@pytest.mark.parametrize("shape,rho", [cc.SWEEP[0], cc.SWEEP[3], cc.SWEEP[9]])
def test_per_sample_identities(shape, rho):
    """Per sample: |R| <= 1 (Cauchy-Schwarz and |c_ab| <= 1, up to the product's rounding), 0 < h < 1, and
    h = 1 - omega s^2: both sides are ss / v resp. 1 - w / v with one division, one square root and one squaring
    between them, a few eps on numbers below 1."""
    for st in qc.oracle_states(shape, rho=rho):
        R, h, s = cc.device_sample(st["Lambda"], st["omega"], rho)
        _, w = cc.rows(st["Lambda"], st["omega"])
        assert np.all(np.abs(R) <= 1.0 + (2 * shape[3] + 8) * cc.EPS)
        assert np.all((h > 0) & (h < 1))
        assert np.max(np.abs(h - (1.0 - w * s * s))) <= 8 * cc.EPS
        assert np.max(np.abs(h - cc.sample_communality(st["Lambda"], st["omega"]))) <= 4 * cc.EPS
        assert np.max(np.abs(R - cc.sample_corr(st["Lambda"], st["omega"], rho))) <= 4 * (shape[3] + 4) * cc.EPS


def test_unpermute_corr_and_communality_round_trip(dcfm):
    rng = np.random.default_rng(8)
    p_orig, p = 11, 9
    keep = np.array([0, 1, 2, 4, 5, 6, 7, 9, 10])            # columns 3 and 8 were dropped
    varind = rng.permutation(p)
    X = rng.standard_normal((30, p))
    S = X.T @ X / 30
    R = dcfm.correlation(S)
    h = rng.uniform(0.1, 0.9, p)
    Rf = dcfm.unpermute_corr(R, keep, varind, p_orig)
    hf = dcfm.unpermute_communality(h, keep, varind, p_orig)
    assert Rf.shape == (p_orig, p_orig) and hf.shape == (p_orig,)
    cols = dcfm.output_columns(keep, varind)
    assert np.array_equal(Rf[np.ix_(cols, cols)], R) and np.array_equal(hf[cols], h)   # no scaling
    assert Rf.tobytes() == dcfm.unpermute_partial(R, keep, varind, p_orig).tobytes()
    for dcol in (3, 8):                                       # a dropped column: the fill, 1 on the diagonal
        off = np.delete(np.arange(p_orig), dcol)
        assert np.isnan(Rf[dcol, off]).all() and np.isnan(Rf[off, dcol]).all() and Rf[dcol, dcol] == 1.0
        assert np.isnan(hf[dcol])
    Z = dcfm.unpermute_corr(R, keep, varind, p_orig, fill=0.0, diag=0.0)
    assert not Z[3].any() and not Z[:, 8].any() and np.array_equal(Z[np.ix_(cols, cols)], R)
    assert dcfm.unpermute_communality(h, keep, varind, p_orig, fill=-1.0)[3] == -1.0
    with pytest.raises(ValueError):
        dcfm.unpermute_communality(np.zeros((p, 2)), keep, varind, p_orig)
    # invariance to the columns' scaling: the correlations of D S D are those of S
    sd = rng.uniform(0.5, 3.0, p)
    assert np.max(np.abs(dcfm.correlation(S * sd[:, None] * sd[None, :]) - R)) < 1e-14


def test_plug_in_correlation_is_not_the_posterior_mean(dcfm):
    """diagnostics.correlation: an exact unit diagonal, NaN where the variance is not positive; and on two
    samples whose variances differ the plug-in of the mean covariance is not the mean of the correlations."""
    S1 = np.array([[1.0, 0.5], [0.5, 1.0]])
    S2 = np.array([[9.0, -1.5], [-1.5, 1.0]])
    R1, R2 = dcfm.correlation(S1), dcfm.diagnostics.correlation(S2)
    assert R1[0, 1] == 0.5 and R2[0, 1] == -0.5
    for R in (R1, R2):
        assert np.array_equal(R.diagonal(), np.ones(2)) and np.array_equal(R, R.T)
    mean_of_corr = 0.5 * (R1 + R2)[0, 1]                       # 0
    plug_in = dcfm.correlation(0.5 * (S1 + S2))[0, 1]          # -0.5 / sqrt(5)
    assert mean_of_corr == 0.0 and plug_in == pytest.approx(-0.5 / np.sqrt(5.0), rel=1e-15)
    X = np.random.default_rng(3).standard_normal((20, 7)) * np.arange(1, 8)
    R = dcfm.correlation(X.T @ X)
    assert np.array_equal(R.diagonal(), np.ones(7)) and np.all(np.abs(R) <= 1 + 4 * cc.EPS)
    bad = dcfm.correlation(np.diag([1.0, 0.0, -2.0]))
    assert bad[0, 0] == 1.0 and np.isnan(bad[1]).all() and np.isnan(bad[:, 2]).all()
    with pytest.raises(ValueError):
        dcfm.correlation(np.zeros((2, 3)))
    # the oracle's chain: the same contrast on real samples, far outside the rounding bound
    states = qc.oracle_states((30, 48, 4, 5), rho=0.5)
    ref = cc.dense_moments(states, 0.5, len(states))
    Sbar = sum(pc.sample_sigma(st["Lambda"], st["omega"], 0.5) for st in states) / len(states)
    gap = float(np.max(np.abs(ref["C"] - dcfm.correlation(Sbar))))
    print(f"max |E R - plug-in| = {gap:.3e}")
    assert gap > 1e3 * ref["b"]


def test_edges_take_the_correlation_moments(dcfm):
    """partial_correlation_edges works on any (mean, sd) pair: here the moments of a correlation matrix."""
    states = qc.oracle_states((30, 48, 4, 5), rho=0.5)
    ref = cc.dense_moments(states, 0.5, len(states))
    e = dcfm.partial_correlation_edges(ref["C"], np.sqrt(np.maximum(ref["var"], 0.0)))
    assert e["edges"].shape == (48, 48) and np.array_equal(e["edges"], e["edges"].T) and not e["edges"].diagonal().any()


def _define(name):
    m = re.search(rf"^#define\s+{name}\s+(0x[0-9a-fA-F]+|\d+)u?\b", HEADER.read_text(), re.M)
    assert m, f"{name} not defined in include/dcfm.h"
    return int(m.group(1), 0)


def test_header_and_binding_agree(dcfm):
    from dcfm_amd import _abi
    assert _define("DCFM_FLAG_CORR") == _abi.DCFM_FLAG_CORR == 0x400
    others = [v for k, v in vars(_abi).items() if k.startswith("DCFM_FLAG_") and k != "DCFM_FLAG_CORR"]
    assert len(others) >= 10 and all(v & _abi.DCFM_FLAG_CORR == 0 for v in others)
    assert _define("DCFM_ABI_VERSION") == 2
    lib = dcfm.load_library()
    vp, DP = C.c_void_p, C.POINTER(C.c_double)
    for name in ("dcfm_get_corr_cols", "dcfm_get_corr", "dcfm_get_communality"):
        assert name in dcfm.EXPORTS and getattr(lib, name).restype is C.c_int
        assert re.search(rf"^int\s+{name}\(", HEADER.read_text(), re.M), name
    assert list(lib.dcfm_get_corr_cols.argtypes) == [vp, C.c_int32, C.c_int64, C.c_int64, DP]
    assert list(lib.dcfm_get_corr.argtypes) == [vp, C.c_int32, DP]
    assert list(lib.dcfm_get_communality.argtypes) == [vp, C.c_int32, DP]
    assert lib.dcfm_abi_version() == 2
    for name in ("correlation", "unpermute_corr", "unpermute_communality"):
        assert name in dcfm.__all__ and callable(getattr(dcfm, name))


def test_null_handle_is_invalid(dcfm):
    from dcfm_amd import _abi
    lib = dcfm.load_library()
    out = (C.c_double * 4)()
    for call in (lambda: lib.dcfm_get_corr_cols(None, 0, 0, 1, out), lambda: lib.dcfm_get_corr(None, 0, out),
                 lambda: lib.dcfm_get_communality(None, 0, out)):
        assert call() == _abi.DCFM_ERR_INVALID
        assert b"null handle" in lib.dcfm_last_error(None)
