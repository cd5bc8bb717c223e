"""CPU tests of the partial correlations (DCFM_FLAG_PARTIAL_CORR, dcfm_get_partial_corr[_cols]): the scaled-panel
restatement of csrc/partial_corr.hip against the dense reference (the partial correlations of the inverse of the
oracle's Sigma(s)) on the oracle's own chain, for every shape of the GPU sweep; diagnostics.partial_correlation_edges
and driver.unpermute_partial; the header and the ctypes binding agree on the new flag and symbols; a null handle
is refused without a GPU."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import partial_corr_cases as rc
import precision_cases as qc
import probe_cases as pc
from helpers import rel_err

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "dcfm.h"


@pytest.mark.parametrize("shape,rho", rc.SWEEP)
def test_scaled_panels_match_the_dense_reference(shape, rho):
    """Bars: entrywise b on the mean and 2 b on the second moment (|t^2 - t_ref^2| <= 2 |t| err, |t| <= 1),
    normwise the project's 1e-10, every kappa_s <= 1e6."""
    states = qc.oracle_states(shape, rho=rho)
    assert len(states) == len(pc.SAVED)
    ref = rc.dense_moments(states, rho, pc.EFFSAMP)
    PC, PC2 = rc.panel_moments(states, rho, pc.EFFSAMP)
    e1, e2 = float(np.max(np.abs(PC - ref["PC"]))), float(np.max(np.abs(PC2 - ref["PC2"])))
    print(f"{shape} rho={rho}: kappa max {max(ref['kappa']):.3e}, b {ref['b']:.3e}, max|PC - ref| {e1:.3e}, "
          f"max|PC2 - ref| {e2:.3e}, rel_err {rel_err(PC, ref['PC']):.3e} / {rel_err(PC2, ref['PC2']):.3e}")
    assert max(ref["kappa"]) <= 1e6
    assert e1 <= ref["b"] and e2 <= 2 * ref["b"]
    assert rel_err(PC, ref["PC"]) < 1e-10 and rel_err(PC2, ref["PC2"]) < 1e-10
    for M in (PC, PC2, ref["PC"], ref["PC2"]):
        assert np.array_equal(M, M.T)
        assert np.array_equal(M.diagonal(), np.full(M.shape[0], len(states) / pc.EFFSAMP))
        assert np.all(np.abs(M) <= len(states) / pc.EFFSAMP)
    assert np.all(ref["var"] >= -4 * ref["b"]) and not ref["var"].diagonal().any()


def test_the_mean_of_the_ratio_is_not_the_ratio_of_the_means(dcfm):
    """What the feature is for: E[R(s)] differs from the plug-in partial correlation of the precision mean."""
    states = qc.oracle_states((30, 48, 4, 5), rho=0.5)
    ref = rc.dense_moments(states, 0.5, len(states))
    Theta = sum(np.linalg.inv(pc.sample_sigma(st["Lambda"], st["omega"], 0.5)) for st in states) / len(states)
    gap = float(np.max(np.abs(ref["PC"] - dcfm.partial_correlations(0.5 * (Theta + Theta.T)))))
    print(f"max |E R - plug-in| = {gap:.3e}")
    assert gap > 1e3 * ref["b"]


def test_partial_correlation_edges(dcfm):
    nan = np.nan
    mean = np.array([[1.0, 0.5, 0.05, 0.0],
                     [0.5, 1.0, -0.4, nan],
                     [0.05, -0.4, 1.0, 0.3],
                     [0.0, nan, 0.3, 1.0]])
    sd = np.array([[0.0, 0.1, 0.01, 0.0],
                   [0.1, 0.0, 0.3, 0.1],
                   [0.01, 0.3, 0.0, 0.0],
                   [0.0, 0.1, 0.0, 0.0]])
    r = dcfm.partial_correlation_edges(mean, sd)
    z, e = r["z"], r["edges"]
    assert e.dtype == bool and e.shape == (4, 4) and np.array_equal(e, e.T) and not e.diagonal().any()
    assert z[0, 1] == 0.5 / 0.1 and z[0, 2] == 0.05 / 0.01 and z[1, 2] == pytest.approx(0.4 / 0.3)
    assert np.isinf(z[2, 3]) and np.isinf(z[0, 0])           # sd == 0, mean != 0
    assert np.isnan(z[0, 3]) and np.isnan(z[1, 3])           # 0 / 0 and a NaN mean
    want = np.zeros((4, 4), dtype=bool)
    for a, b in ((0, 1), (0, 2), (2, 3)):                    # z = 5, 5, inf; (1, 2) has z = 1.33; NaN -> False
        want[a, b] = want[b, a] = True
    assert np.array_equal(e, want)
    e2 = dcfm.diagnostics.partial_correlation_edges(mean, sd, z=1.0, min_abs=0.1)["edges"]
    want[0, 2] = want[2, 0] = False                          # |mean| = 0.05 < min_abs
    want[1, 2] = want[2, 1] = True                           # z = 1.33 >= 1
    assert np.array_equal(e2, want)
    with pytest.raises(ValueError):
        dcfm.partial_correlation_edges(mean, sd[:3, :3])


def test_unpermute_partial_round_trips_against_unpermute_sigma(dcfm):
    rng = np.random.default_rng(8)
    p_orig, p = 11, 9
    keep = np.array([0, 1, 2, 4, 5, 6, 7, 9, 10])            # columns 3 and 8 were dropped
    varind = rng.permutation(p)
    X = rng.standard_normal((30, p))
    T = np.linalg.inv(X.T @ X / 30)
    R = dcfm.partial_correlations(0.5 * (T + T.T))
    Rf = dcfm.unpermute_partial(R, keep, varind, p_orig)
    assert Rf.shape == (p_orig, p_orig)
    Sf = dcfm.unpermute_sigma(R, keep, varind, p_orig, sd=None, fill=np.nan)
    kept = np.ix_(keep, keep)
    assert np.array_equal(Rf[kept], Sf[kept]) and not np.isnan(Rf[kept]).any()
    cols = dcfm.output_columns(keep, varind)
    assert np.array_equal(Rf[np.ix_(cols, cols)], R)          # the permutation undone, no scaling
    for dcol in (3, 8):                                       # a dropped column: the fill, 1 on the diagonal
        off = np.delete(np.arange(p_orig), dcol)
        assert np.isnan(Rf[dcol, off]).all() and np.isnan(Rf[off, dcol]).all() and Rf[dcol, dcol] == 1.0
    Z = dcfm.unpermute_partial(R, keep, varind, p_orig, fill=0.0)
    assert not Z[3, np.arange(p_orig) != 3].any() and Z[3, 3] == 1.0 and np.array_equal(Z[kept], Rf[kept])
    # invariance to the columns' scaling: the partial correlations of D T D are those of T
    sd = rng.uniform(0.5, 3.0, p)
    assert np.max(np.abs(dcfm.partial_correlations(T / sd[:, None] / sd[None, :]) - R)) < 1e-14


def _define(name):
    m = re.search(rf"^#define\s+{name}\s+(0x[0-9a-fA-F]+|\d+)u?\b", HEADER.read_text(), re.M)
    assert m, f"{name} not defined in include/dcfm.h"
    return int(m.group(1), 0)


def test_header_and_binding_agree(dcfm):
    from dcfm_amd import _abi
    assert _define("DCFM_FLAG_PARTIAL_CORR") == _abi.DCFM_FLAG_PARTIAL_CORR == 0x200
    others = [v for k, v in vars(_abi).items() if k.startswith("DCFM_FLAG_") and k != "DCFM_FLAG_PARTIAL_CORR"]
    assert len(others) >= 9 and all(v & _abi.DCFM_FLAG_PARTIAL_CORR == 0 for v in others)
    assert _define("DCFM_ABI_VERSION") == 2
    lib = dcfm.load_library()
    vp, DP = C.c_void_p, C.POINTER(C.c_double)
    assert "dcfm_get_partial_corr_cols" in dcfm.EXPORTS and "dcfm_get_partial_corr" in dcfm.EXPORTS
    assert lib.dcfm_get_partial_corr_cols.restype is C.c_int and lib.dcfm_get_partial_corr.restype is C.c_int
    assert list(lib.dcfm_get_partial_corr_cols.argtypes) == [vp, C.c_int32, C.c_int64, C.c_int64, DP]
    assert list(lib.dcfm_get_partial_corr.argtypes) == [vp, C.c_int32, DP]
    hdr = HEADER.read_text()
    for name in ("dcfm_get_partial_corr_cols", "dcfm_get_partial_corr"):
        assert re.search(rf"^int\s+{name}\(", hdr, re.M), name
    assert lib.dcfm_abi_version() == 2
    for name, w in (("mean", 0), ("m2", 1), ("sd", 2)):
        assert dcfm.Sampler._moment(name) == w
    with pytest.raises(ValueError):
        dcfm.Sampler._moment("var")


def test_null_handle_is_invalid(dcfm):
    from dcfm_amd import _abi
    lib = dcfm.load_library()
    out = (C.c_double * 4)()
    assert lib.dcfm_get_partial_corr_cols(None, 0, 0, 1, out) == _abi.DCFM_ERR_INVALID
    assert b"null handle" in lib.dcfm_last_error(None)
    assert lib.dcfm_get_partial_corr(None, 0, out) == _abi.DCFM_ERR_INVALID
    assert b"null handle" in lib.dcfm_last_error(None)
