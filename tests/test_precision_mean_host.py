"""CPU tests of the precision mean (DCFM_FLAG_PRECISION_MEAN, dcfm_get_precision_mean[_cols]): the NumPy
restatements of the factor forms of csrc/precision_mean.hip against the dense inverse of the oracle's
Sigma(s) on the oracle's chain states at rho = 0, 0.5 and 1; diagnostics.partial_correlations and
driver.unpermute_precision; the header and the ctypes binding agree on the new flag and symbols; a null
handle is refused without a GPU."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import precision_cases as qc
import precision_mean_cases as mc
import probe_cases as pc
from helpers import rel_err

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "dcfm.h"

# (n, p, g, K): one partial tile; K = 1; P = 100 (mixed tiles on the device); the wide state layout
SHAPES = [(30, 48, 4, 5), (30, 36, 3, 1), (37, 300, 3, 7), (40, 99, 3, 33)]


@pytest.mark.parametrize("rho", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("shape", SHAPES)
def test_factor_forms_match_the_dense_inverse(shape, rho):
    states = qc.oracle_states(shape, rho=rho)
    assert len(states) == len(pc.SAVED)
    ref = mc.dense_mean(states, rho, pc.EFFSAMP)
    P = states[0]["Lambda"].shape[0]
    sym = sum(mc.sample_precision(st["Lambda"], st["omega"], rho) for st in states) / pc.EFFSAMP
    two = sum(mc.from_panels(*mc.panels(st["Lambda"], st["omega"], rho), P) for st in states) / pc.EFFSAMP
    for name, T in (("A / Gamma", sym), ("two panels", two)):
        r, e = mc.ratio(T, ref), rel_err(T, ref["T"])
        print(f"{shape} rho={rho} {name}: kappa max {max(ref['kappa']):.3e}, err / bound {r:.4f}, rel_err {e:.3e}")
        assert max(ref["kappa"]) <= 1e6
        assert r <= 1.0 and e < 1e-10
        assert np.array_equal(T, T.T) and np.all(T.diagonal() > 0)
    if rho == 0.0:                                           # no cross-shard term: Gamma = 0 exactly
        assert not mc.factors(states[0]["Lambda"], states[0]["omega"], rho)[2].any()
    if rho == 1.0:                                           # no same-shard term: A = 0 exactly
        assert not mc.factors(states[0]["Lambda"], states[0]["omega"], rho)[1].any()


def test_partial_correlations(dcfm):
    T = np.array([[4.0, -1.2], [-1.2, 1.0]])                 # 2 x 2: r = 1.2 / (sqrt(4) sqrt(1)) = 0.6
    R = dcfm.partial_correlations(T)
    assert np.array_equal(R, [[1.0, 0.6], [0.6, 1.0]])
    rng = np.random.default_rng(3)
    X = rng.standard_normal((40, 9))
    T = np.linalg.inv(X.T @ X / 40)
    T = 0.5 * (T + T.T)
    R = dcfm.diagnostics.partial_correlations(T)
    assert np.array_equal(R, R.T) and np.array_equal(R.diagonal(), np.ones(9))
    assert np.all(np.abs(R) <= 1.0 + 1e-15)
    assert R[2, 5] == pytest.approx(-T[2, 5] / np.sqrt(T[2, 2] * T[5, 5]), rel=1e-15)
    with pytest.raises(ValueError):
        dcfm.partial_correlations(np.zeros((2, 3)))


@pytest.mark.parametrize("with_sd", [False, True])
def test_unpermute_precision_inverts_unpermute_sigma(dcfm, with_sd):
    rng = np.random.default_rng(8)
    p_orig, p = 11, 9
    keep = np.array([0, 1, 2, 4, 5, 6, 7, 9, 10])            # columns 3 and 8 were dropped
    varind = rng.permutation(p)
    X = rng.standard_normal((30, p))
    S = X.T @ X / 30
    T = np.linalg.inv(S)
    sd = rng.uniform(0.5, 3.0, p) if with_sd else None
    Sf = dcfm.unpermute_sigma(S, keep, varind, p_orig, sd=sd)
    Tf = dcfm.unpermute_precision(T, keep, varind, p_orig, sd=sd)
    assert Tf.shape == (p_orig, p_orig)
    assert not Tf[3].any() and not Tf[:, 8].any()            # dropped columns: the fill
    assert np.max(np.abs(Sf[np.ix_(keep, keep)] @ Tf[np.ix_(keep, keep)] - np.eye(p))) < 1e-10
    cols = dcfm.output_columns(keep, varind)
    a, b = 2, 7
    want = T[a, b] / sd[a] / sd[b] if with_sd else T[a, b]
    assert Tf[cols[a], cols[b]] == want
    assert dcfm.unpermute_precision(T, keep, varind, p_orig, fill=np.nan)[3, 3] != 0.0   # NaN fill


def _define(name):
    m = re.search(rf"^#define\s+{name}\s+(0x[0-9a-fA-F]+|\d+)u?\b", HEADER.read_text(), re.M)
    assert m, f"{name} not defined in include/dcfm.h"
    return int(m.group(1), 0)


def test_header_and_binding_agree(dcfm):
    from dcfm_amd import _abi
    assert _define("DCFM_FLAG_PRECISION_MEAN") == _abi.DCFM_FLAG_PRECISION_MEAN == 0x100
    others = [v for k, v in vars(_abi).items() if k.startswith("DCFM_FLAG_") and k != "DCFM_FLAG_PRECISION_MEAN"]
    assert len(others) >= 8 and all(v & _abi.DCFM_FLAG_PRECISION_MEAN == 0 for v in others)
    assert _define("DCFM_ABI_VERSION") == 2 and _define("DCFM_K_COUNT") == _abi.K_COUNT == 15
    lib = dcfm.load_library()
    vp, DP = C.c_void_p, C.POINTER(C.c_double)
    assert "dcfm_get_precision_mean_cols" in dcfm.EXPORTS and "dcfm_get_precision_mean" in dcfm.EXPORTS
    assert lib.dcfm_get_precision_mean_cols.restype is C.c_int and lib.dcfm_get_precision_mean.restype is C.c_int
    assert list(lib.dcfm_get_precision_mean_cols.argtypes) == [vp, C.c_int64, C.c_int64, DP]
    assert list(lib.dcfm_get_precision_mean.argtypes) == [vp, DP]
    hdr = HEADER.read_text()
    for name in ("dcfm_get_precision_mean_cols", "dcfm_get_precision_mean"):
        assert re.search(rf"^int\s+{name}\(", hdr, re.M), name
    assert lib.dcfm_abi_version() == 2


def test_null_handle_is_invalid(dcfm):
    from dcfm_amd import _abi
    lib = dcfm.load_library()
    out = (C.c_double * 4)()
    assert lib.dcfm_get_precision_mean_cols(None, 0, 1, out) == _abi.DCFM_ERR_INVALID
    assert b"null handle" in lib.dcfm_last_error(None)
    assert lib.dcfm_get_precision_mean(None, out) == _abi.DCFM_ERR_INVALID
    assert b"null handle" in lib.dcfm_last_error(None)
