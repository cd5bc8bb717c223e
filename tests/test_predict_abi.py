"""CPU tests of the conditional prediction's boundary (dcfm_set_predict / dcfm_get_predict): the binding lists
and resolves both symbols (five and seven arguments), a null handle is refused with nothing written, the ABI
version and the kernel-id count stay (the change is additive), the Sampler methods, the driver's argument and the
diagnostics export exist, the driver's unit conversion round-trips on a small Y with a dropped column, and
diagnostics.conditional_log_density agrees with a direct evaluation -- all without a GPU."""
import ctypes as C
import inspect
import re
from pathlib import Path

import numpy as np
import pytest
from scipy.stats import multivariate_normal

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "dcfm.h"


def _define(name):
    m = re.search(rf"^#define\s+{name}\s+(0x[0-9a-fA-F]+|\d+)u?\b", HEADER.read_text(), re.M)
    assert m, f"{name} not defined in include/dcfm.h"
    return int(m.group(1), 0)


def test_library_resolves_the_new_symbols(dcfm):
    lib = dcfm.load_library()
    for name, nargs in (("dcfm_set_predict", 5), ("dcfm_get_predict", 7)):
        assert name in dcfm.EXPORTS
        assert re.search(rf"\bint\s+{name}\s*\(", HEADER.read_text()), f"{name} not declared in include/dcfm.h"
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == nargs


def test_the_change_is_additive(dcfm):
    from dcfm_amd import _abi
    lib = dcfm.load_library()
    assert _define("DCFM_ABI_VERSION") == 2 == lib.dcfm_abi_version()
    assert _define("DCFM_K_COUNT") == _abi.K_COUNT == 15 == len(_abi.KERNEL_IDS)


def test_null_handle_is_invalid(dcfm):
    from dcfm_amd import _abi
    lib = dcfm.load_library()
    y, ob = (C.c_double * 4)(), (C.c_uint8 * 4)()
    assert lib.dcfm_set_predict(None, y, ob, 1, 3) == _abi.DCFM_ERR_INVALID
    assert b"null handle" in lib.dcfm_last_error(None)
    bufs = [(C.c_double * 4)() for _ in range(5)]
    cnt = C.c_int64(-7)
    assert lib.dcfm_get_predict(None, *bufs, C.byref(cnt)) == _abi.DCFM_ERR_INVALID
    assert b"null handle" in lib.dcfm_last_error(None)
    assert all(list(b) == [0.0] * 4 for b in bufs) and cnt.value == -7


def test_python_surface_exists(dcfm):
    assert callable(dcfm.Sampler.set_predict) and callable(dcfm.Sampler.predict)
    assert "conditional_log_density" in dcfm.__all__
    assert dcfm.conditional_log_density is dcfm.diagnostics.conditional_log_density
    par = inspect.signature(dcfm.divideconquer).parameters
    assert "predict" in par and par["predict"].default is None
    assert list(par)[list(par).index("loglik") + 1] == "predict"
    assert "set_predict" in dcfm.divideconquer.__doc__
    for word in ("sd_total", "sd_between", "cvar", "maha", "logdet", "count"):
        assert word in dcfm.Sampler.predict.__doc__, word
    for word in ("standardised", "log sd_j"):                    # the units
        assert word in dcfm.conditional_log_density.__doc__, word
    assert "DCFM_ERR_UNSUPPORTED" in dcfm.Sampler.set_predict.__doc__


def test_unit_conversion_round_trips(dcfm):
    """A small Y with a dropped all-zero column: standardize_rows centres, scales and permutes; pushing the
    standardised rows back as a 'prediction' through unstandardize_prediction returns the data on the observed
    kept columns, the training mean where yhat is zero, and 0 on the dropped column."""
    drv = dcfm.driver
    rng = np.random.default_rng(3)
    n, p0, nt = 12, 7, 3
    Y = rng.standard_normal((n, p0)) * rng.uniform(0.5, 3.0, p0) + rng.uniform(-2, 2, p0)
    Y[:, 2] = 0.0
    Yk, _, p, P, K, keep = drv.preprocess(Y, 2, 2)
    assert p == 6 and 2 not in keep
    varind = rng.permutation(p)
    cols = drv.output_columns(keep, varind)
    mean, sd = drv.column_moments(Y)
    assert sd[2] == 0.0 and mean[2] == 0.0 and np.allclose(sd[keep], Yk.std(axis=0, ddof=1), rtol=1e-15)
    Ynew = rng.standard_normal((nt, p0))
    obs = np.array([True, False, True, True, False, True, True])
    Ynew[:, ~obs] = np.nan                                       # ignored wherever unobserved
    Ystd, ob = drv.standardize_rows(Ynew, obs, mean, sd, keep, varind)
    assert Ystd.shape == (p, nt) and ob.dtype == np.uint8 and ob.shape == (p,)
    assert np.array_equal(ob != 0, obs[cols]) and ob.sum() == obs.sum() - 1     # the dropped column is unobserved
    assert np.all(np.isfinite(Ystd)) and not Ystd[ob == 0].any()
    assert np.array_equal(Ystd[ob != 0], ((Ynew[:, cols[ob != 0]] - mean[cols[ob != 0]]) / sd[cols[ob != 0]]).T)
    # the same standardisation as the training data's (dc:57-59)
    Ytr, _ = drv.standardize_rows(Y, np.ones(p0, bool), mean, sd, keep, varind)
    ref = drv.partition_standardize(Yk, 2, varind)               # n x P x g
    assert np.allclose(Ytr.T, np.concatenate([ref[:, :, m] for m in range(2)], axis=1), rtol=1e-13, atol=1e-13)
    one, _ = drv.standardize_rows(Ynew[0], obs, mean, sd, keep, varind)         # a single row: (p_orig,)
    assert np.array_equal(one[:, 0], Ystd[:, 0])
    pred = {"mean": Ystd, "sd_between": np.full((p, nt), 0.5), "sd_total": np.ones((p, nt))}
    back = drv.unstandardize_prediction(pred, mean, sd, keep, varind, p0)
    assert back["mean"].shape == (nt, p0) == back["sd_total"].shape
    ko = obs.copy()
    ko[2] = False
    assert np.allclose(back["mean"][:, ko], Ynew[:, ko], rtol=1e-13, atol=1e-13)
    un = ~obs
    assert np.array_equal(back["mean"][:, un], np.broadcast_to(mean[un], (nt, un.sum())))
    assert not back["mean"][:, 2].any() and not back["sd_total"][:, 2].any() and not back["sd_between"][:, 2].any()
    assert np.array_equal(back["sd_total"][:, keep], np.broadcast_to(sd[keep], (nt, p)))
    assert np.array_equal(back["sd_between"][:, keep], np.broadcast_to(0.5 * sd[keep], (nt, p)))
    with pytest.raises(ValueError):
        drv.standardize_rows(Ynew[:, :5], obs, mean, sd, keep, varind)


def test_conditional_log_density_against_a_direct_evaluation(dcfm):
    rng = np.random.default_rng(8)
    S, nt, na = 4, 3, 5
    ya = rng.standard_normal((na, nt))
    maha, ld, direct = np.zeros((S, nt)), np.zeros(S), np.zeros((S, nt))
    for s in range(S):
        A = rng.standard_normal((na, na + 2))
        Sig = A @ A.T + 0.5 * np.eye(na)
        maha[s] = np.einsum("at,at->t", ya, np.linalg.solve(Sig, ya))
        ld[s] = np.linalg.slogdet(Sig)[1]
        direct[s] = multivariate_normal(np.zeros(na), Sig).logpdf(ya.T)
    r = dcfm.conditional_log_density(maha, ld, na)
    assert r["per_sample"].shape == (S, nt) and np.allclose(r["per_sample"], direct, rtol=1e-12, atol=1e-12)
    want = np.log(np.mean(np.exp(direct), axis=0))
    assert np.allclose(r["lppd"], want, rtol=1e-12) and r["total"] == pytest.approx(want.sum(), rel=1e-12)
    far = dcfm.conditional_log_density(np.array([[4000.0], [4002.0]]), np.zeros(2), 1)   # no underflow
    assert far["lppd"][0] == pytest.approx(-0.5 * np.log(2 * np.pi) - 2000.0 + np.log((1 + np.exp(-1.0)) / 2), rel=1e-15)
    none = dcfm.conditional_log_density(np.zeros((3, 0)), np.zeros(3), 0)                # nt = 0
    assert none["lppd"].shape == (0,) and none["total"] == 0.0
    with pytest.raises(ValueError):
        dcfm.conditional_log_density(np.zeros((2, 1)), np.zeros(3), 2)
