"""The largest eigenpairs of Sigmaout on the device (dcfm_sigma_eigs: block Krylov on dcfm_sigma_apply,
Rayleigh-Ritz on the host) against numpy.linalg.eigvalsh of the read-back matrix.

With the default max_passes the basis can reach the full dimension, so convergence does not rest on
an iteration count.  Bounds: a residual bounds the distance to an eigenvalue, so each value is within
tol lambda_1 + 4 p eps lambda_1 of the host's (the second term: the host reference's own rounding);
two-pass Gram-Schmidt leaves V'V - I at O(eps), asserted <= 1e-12; the residual recomputed on the host
is <= 2 tol lambda_1 and agrees with the returned one to 4 p eps lambda_1.
"""
import numpy as np
import pytest

from helpers import make_case, state_dict
from sigma_cases import cases, loopback_pair  # noqa: F401  (cases: a fixture)

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
TOL = 1e-10


def _check(res, S, r, tol=TOL):
    p = S.shape[0]
    lam = np.linalg.eigvalsh(S)[::-1]
    l1 = lam[0]
    vals, V, rs = res["values"], res["vectors"], res["resid"]
    assert vals.shape == (r,) and V.shape == (p, r) and rs.shape == (r,)
    print(f"p={p} r={r}: passes {res['passes']}, max resid / lambda_1 {float(np.max(rs)) / l1:.3e}, "
          f"max |values - eigvalsh| / lambda_1 {float(np.max(np.abs(vals - lam[:r]))) / l1:.3e}")
    assert res["converged"] is True
    assert np.all(np.diff(vals) <= 0)
    assert np.all(np.abs(vals - lam[:r]) <= tol * l1 + 4 * p * EPS * l1)
    assert np.max(np.abs(V.T @ V - np.eye(r))) <= 1e-12
    host = np.linalg.norm(S @ V - V * vals[None, :], axis=0)
    assert np.all(host <= 2 * tol * l1)
    assert np.all(np.abs(host - rs) <= 4 * p * EPS * l1)
    big = np.argmax(np.abs(V), axis=0)                       # first index of the largest magnitude
    assert np.all(V[big, np.arange(r)] > 0)


@pytest.mark.parametrize("shape", [(60, 150, 5, 3), (60, 384, 4, 4)])
def test_leading_pairs_match_a_host_eigensolve(cases, shape):
    smp, S = cases(shape)
    res = smp.sigma_eigs(6, tol=TOL)
    _check(res, S, 6)
    again = smp.sigma_eigs(6, tol=TOL)
    for k in ("values", "vectors", "resid"):
        assert np.array_equal(res[k], again[k]), k            # same seed: the same bits
    assert again["passes"] == res["passes"]
    nov = smp.sigma_eigs(6, tol=TOL, vectors=False)
    assert nov["vectors"] is None and np.array_equal(nov["values"], res["values"])
    _check(smp.sigma_eigs(1, tol=TOL), S, 1)


def test_full_block_width(cases):
    smp, S = cases((60, 384, 4, 4))
    _check(smp.sigma_eigs(32, tol=TOL), S, 32)


def test_whole_spectrum_of_a_small_matrix(cases):
    """r = p = 30: the start block spans everything, exact after the first pass."""
    smp, S = cases((40, 30, 3, 2))
    res = smp.sigma_eigs(30, tol=TOL)
    assert res["passes"] == 1
    _check(res, S, 30)


def test_unconverged_is_not_an_error(cases):
    smp, S = cases((60, 384, 4, 4))
    res = smp.sigma_eigs(6, tol=1e-6, max_passes=2)
    assert 1 <= res["passes"] <= 2
    assert res["converged"] == bool(np.all(res["resid"] <= 1e-6 * res["values"][0]))
    assert np.all(np.isfinite(res["values"])) and np.all(np.isfinite(res["vectors"]))
    host = np.linalg.norm(S @ res["vectors"] - res["vectors"] * res["values"][None, :], axis=0)
    assert np.all(np.abs(host - res["resid"]) <= 4 * 384 * EPS * np.linalg.eigvalsh(S)[-1])


def test_arguments(cases, dcfm):
    from dcfm_amd import _abi
    smp, _ = cases((60, 150, 5, 3))
    for kw in (dict(r=0), dict(r=33), dict(r=6, tol=0.0), dict(r=6, tol=-1.0), dict(r=6, max_passes=0)):
        with pytest.raises(dcfm.DcfmError) as e:
            smp.sigma_eigs(**kw)
        assert e.value.code == _abi.DCFM_ERR_INVALID, kw
    small, _ = cases((40, 30, 3, 2))
    with pytest.raises(dcfm.DcfmError) as e:
        small.sigma_eigs(31)                                  # r > p
    assert e.value.code == _abi.DCFM_ERR_INVALID


def test_no_saved_sample_is_invalid(dcfm):
    from dcfm_amd import _abi
    c = make_case(40, 30, 3, 2, seed=21, k0=4)
    smp = dcfm.Sampler(c["n"], c["P"], 3, 2, c["rho"], 5, 4, 1, seed=7)
    try:
        smp.set_data(c["Yd"])
        smp.set_state({k: v for k, v in state_dict(c["st"]).items() if k != "eta"})
        smp.run(1, 3)                                         # still inside the burn-in
        assert smp.saved_samples() == 0
        with pytest.raises(dcfm.DcfmError) as e:
            smp.sigma_eigs(3)
        assert e.value.code == _abi.DCFM_ERR_INVALID and "saved sample" in str(e.value)
    finally:
        smp.close()


def test_loopback_ranks_return_the_same_bits(dcfm):
    def work(r, smp):
        return smp.get_sigma(), smp.sigma_eigs(6, tol=TOL)

    (S, e0), (_, e1) = loopback_pair(dcfm, work)
    for k in ("values", "vectors", "resid"):
        assert np.array_equal(e0[k], e1[k]), k
    assert e0["passes"] == e1["passes"]
    _check(e0, S, 6)


def test_driver_components_and_unpermute_vectors(dcfm):
    n, p, g, K = 60, 150, 5, 3
    c = make_case(n, p, g, K, seed=21, k0=4, zero_cols=0)
    S, pcs, info = dcfm.divideconquer(c["Y"], g, K * g, 2, 6, 2, 0.5, seed=3, n_components=3, return_info=True)
    assert set(pcs) == {"values", "vectors", "resid", "passes", "converged"}
    _check(pcs, S, 3)
    # back in the input's column order: unpermute_sigma(S) times the unpermuted vector is lambda times it
    p0 = c["Y"].shape[1]
    Su = dcfm.unpermute_sigma(S, info["keep"], info["varind"], p0)
    Vu = dcfm.unpermute_vectors(pcs["vectors"], info["keep"], info["varind"], p0)
    assert Vu.shape == (p0, 3)
    kept = dcfm.output_columns(info["keep"], info["varind"])
    apply_bound = 4 * p * EPS * (np.abs(Su) @ np.abs(Vu))
    # a pure permutation: the product in the input's order is the permuted product, up to summation order
    SVu = dcfm.unpermute_vectors(S @ pcs["vectors"], info["keep"], info["varind"], p0)
    assert np.all(np.abs(Su @ Vu - SVu)[kept] <= apply_bound[kept])
    # and lambda times the vector, up to the pair's own residual (|r_a| <= ||r||_2) on top of that bound
    bound = apply_bound + pcs["resid"][None, :]
    assert np.all(np.abs(Su @ Vu - Vu * pcs["values"][None, :])[kept] <= bound[kept])
    assert np.array_equal(dcfm.unpermute_vectors(pcs["vectors"][:, 0], info["keep"], info["varind"], p0), Vu[:, 0])
    # the default leaves the returned tuple as it was
    out = dcfm.divideconquer(c["Y"], g, K * g, 2, 6, 2, 0.5, seed=3, return_info=True)
    assert len(out) == 2 and out[0].shape == S.shape and isinstance(out[1], dict) and "varind" in out[1]
