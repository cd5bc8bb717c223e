"""X = Sigmaout^{-1} B on the device (dcfm_sigma_solve, csrc/sigma_solve.hip: conjugate gradients, every
column on its own, the whole iteration in HBM) against the read-back matrix S.

Shapes (n, p, g, K) as in test_gpu_sigma_apply.py: (40, 30, 3, 2) p smaller than a wave; (60, 150, 5, 3)
p no multiple of 64; (60, 384, 4, 4) three exact tile rows; (60, 400, 4, 5) on two loopback ranks.
tol = 1e-8, kappa = cond_2(S) by NumPy, eps = 2^-52.

* Residual: the host's ||B_c - S X_c|| / ||B_c|| <= tol + 4 iters_c p eps kappa (the gap between the
  recurrence's residual, which meets tol, and the true one), and it agrees with the returned relres
  within 4 p eps (|| |S| |X_c| || + ||B_c||) / ||B_c|| (two evaluations of the same residual).
* Forward error: ||X_c - Xref_c|| <= (kappa relres_c + p eps kappa) ||Xref_c||, Xref = numpy.linalg.solve
  (the first term: a residual bounds the error by kappa; the second: the reference's own error).
* Columns of S as right-hand sides give the identity's columns within that bound.
* quad = the column sums of B o X within p eps sum |B| |X|.
* iters_c <= the count of a NumPy restatement of the same recurrence on S, plus 2 (summation order can
  move the threshold crossing).
* A zero column: X exactly 0, relres 0, iters 0, the others bitwise unchanged; max_iter is no error.
* The same input gives the same bytes; a column's bits do not depend on its neighbours (also in the
  second chunk of 32); DCFM_FLAG_SIGMA_M2 changes nothing; two ranks return the same bytes.
"""
import ctypes as C

import numpy as np
import pytest

from helpers import make_case, state_dict
from sigma_cases import cases, loopback_pair, run_sampler  # noqa: F401  (cases: a fixture)

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
TOL = 1e-8
SHAPES = [(40, 30, 3, 2), (60, 150, 5, 3), (60, 384, 4, 4)]
NVS = (1, 5, 17, 32, 40)                         # 40: two chunks inside the call
_kappa = {}


def kappa(S):
    key = (S.shape[0], float(S[0, 0]), float(S[-1, 0]))
    if key not in _kappa:
        _kappa[key] = float(np.linalg.cond(S))
    return _kappa[key]


def cg_reference(S, B, tol, max_iter):
    """The recurrence of csrc/sigma_solve.hip in NumPy, every column on its own: steps taken per column."""
    X, R, P = np.zeros_like(B), B.copy(), B.copy()
    bb = np.einsum("ij,ij->j", B, B)
    rr = bb.copy()
    done = ~(bb > 0)
    iters = np.zeros(B.shape[1], dtype=np.int64)
    for _ in range(max_iter):
        if done.all():
            break
        W = S @ P
        pw = np.einsum("ij,ij->j", P, W)
        live = ~done & (pw > 0) & np.isfinite(pw)
        alpha = np.where(live, rr / np.where(live, pw, 1.0), 0.0)
        X += P * alpha
        R -= W * alpha
        rn = np.where(live, np.einsum("ij,ij->j", R, R), rr)
        done = ~live | (np.sqrt(rn) <= tol * np.sqrt(bb))
        beta = np.where(done, 0.0, rn / np.where(rr > 0, rr, 1.0))
        P = np.where(done, P, R + P * beta)
        iters += live
        rr = rn
    return iters


def check_solution(S, B, X, info, tol=TOL):
    """The residual, forward-error, quad and iteration-count assertions of the module docstring."""
    p, nv = B.shape
    k = kappa(S)
    nb = np.linalg.norm(B, axis=0)
    relres, iters, quad = info["relres"], info["iters"], info["quad"]
    assert X.shape == B.shape and relres.shape == iters.shape == quad.shape == (nv,)
    host = np.linalg.norm(B - S @ X, axis=0) / nb
    gap = 4.0 * p * EPS * (np.linalg.norm(np.abs(S) @ np.abs(X), axis=0) + nb) / nb
    Xref = np.linalg.solve(S, B)
    ferr = np.linalg.norm(X - Xref, axis=0)
    fbound = (k * relres + p * EPS * k) * np.linalg.norm(Xref, axis=0)
    qref, qbound = np.sum(B * X, axis=0), p * EPS * np.sum(np.abs(B) * np.abs(X), axis=0)
    ref_iters = cg_reference(S, B, tol, min(2 * p, 1000))
    print(f"p={p} nv={nv} kappa={k:.1f}: iters {iters.min()}..{iters.max()} (reference {ref_iters.min()}.."
          f"{ref_iters.max()}), max host relres {host.max():.3e}, max |host - relres| / bound "
          f"{np.max(np.abs(host - relres) / gap):.3e}, max forward err / bound {np.max(ferr / fbound):.3e}, "
          f"max quad err / bound {np.max(np.abs(quad - qref) / qbound):.3e}")
    assert np.all(host <= tol + 4.0 * iters * p * EPS * k)
    assert np.all(np.abs(host - relres) <= gap)
    assert np.all(ferr <= fbound)
    assert np.all(np.abs(quad - qref) <= qbound)
    assert np.all(iters <= ref_iters + 2) and np.all(iters >= 1)
    assert np.array_equal(info["converged"], iters < min(2 * p, 1000)) and info["converged"].all()


@pytest.mark.parametrize("shape", SHAPES)
def test_random_right_hand_sides(cases, shape):
    smp, S = cases(shape)
    p = shape[1]
    rng = np.random.default_rng(6)
    for nv in NVS:
        B = rng.standard_normal((p, nv))
        X, info = smp.sigma_solve(B, tol=TOL, return_info=True)
        check_solution(S, B, X, info)
        assert info["ms"] > 0.0
        X2, info2 = smp.sigma_solve(B, tol=TOL, return_info=True)
        assert np.array_equal(X2, X), "same input, different bytes"
        for f in ("relres", "iters", "quad"):
            assert np.array_equal(info2[f], info[f]), f


def _starts(p, nv):
    """First columns: 0, across the 128 boundary where p allows, the last ones."""
    out = {0, p - nv}
    if p >= 120 + nv:
        out.add(120)
    return sorted(c for c in out if 0 <= c <= p - nv)


@pytest.mark.parametrize("shape", SHAPES)
def test_columns_of_sigma_give_identity_columns(cases, shape):
    smp, S = cases(shape)
    p = shape[1]
    k = kappa(S)
    for nv in (1, 17):
        for c0 in _starts(p, nv):
            B = np.asfortranarray(S[:, c0:c0 + nv])
            X, info = smp.sigma_solve(B, tol=TOL, return_info=True)
            E = np.zeros((p, nv))
            E[c0 + np.arange(nv), np.arange(nv)] = 1.0
            err = np.linalg.norm(X - E, axis=0)
            bound = k * info["relres"] + p * EPS * k                     # ||e_c|| = 1
            print(f"{shape} nv={nv} c0={c0}: max err / bound {np.max(err / bound):.3e}")
            assert np.all(err <= bound), (shape, nv, c0)
            check_solution(S, B, X, info)


def test_vector_shapes_and_defaults(cases):
    smp, S = cases((60, 150, 5, 3))
    p = 150
    b = np.random.default_rng(2).standard_normal(p)
    x = smp.sigma_solve(b)                                               # tol 1e-10, max_iter min(2 p, 1000)
    assert x.shape == (p,)
    x2, info = smp.sigma_solve(b, return_info=True)
    assert np.array_equal(x2, x)
    assert isinstance(info["relres"], float) and isinstance(info["iters"], int) and info["converged"] is True
    assert info["relres"] <= 1e-10 + 4.0 * info["iters"] * p * EPS * kappa(S)
    assert np.array_equal(smp.sigma_solve(b[:, None])[:, 0], x)
    Bc = np.ascontiguousarray(np.random.default_rng(3).standard_normal((p, 7)))    # C order in, same result
    assert np.array_equal(smp.sigma_solve(Bc, tol=TOL), smp.sigma_solve(np.asfortranarray(Bc), tol=TOL))


def test_zero_column_and_max_iter(cases):
    smp, S = cases((60, 384, 4, 4))
    p = 384
    B = np.random.default_rng(11).standard_normal((p, 5))
    X, info = smp.sigma_solve(B, tol=TOL, return_info=True)
    Bz = B.copy()
    Bz[:, 2] = 0.0
    Xz, iz = smp.sigma_solve(Bz, tol=TOL, return_info=True)
    assert np.array_equal(Xz[:, 2], np.zeros(p)) and not np.any(np.signbit(Xz[:, 2]))
    assert iz["relres"][2] == 0.0 and iz["iters"][2] == 0 and iz["quad"][2] == 0.0
    keep = [0, 1, 3, 4]
    assert np.array_equal(Xz[:, keep], X[:, keep])                       # the others: bitwise what they were
    for f in ("relres", "iters", "quad"):
        assert np.array_equal(iz[f][keep], info[f][keep]), f
    Z, zi = smp.sigma_solve(np.zeros((p, 3)), tol=TOL, return_info=True)  # nothing but zero columns
    assert np.array_equal(Z, np.zeros((p, 3))) and not zi["iters"].any() and not zi["relres"].any()
    X3, i3 = smp.sigma_solve(B, tol=TOL, max_iter=3, return_info=True)    # unconverged is not an error
    assert np.all(i3["iters"] == 3) and np.all(i3["relres"] > TOL) and not i3["converged"].any()
    assert np.all(np.isfinite(X3))
    host = np.linalg.norm(B - S @ X3, axis=0) / np.linalg.norm(B, axis=0)
    gap = 4.0 * p * EPS * (np.linalg.norm(np.abs(S) @ np.abs(X3), axis=0) / np.linalg.norm(B, axis=0) + 1.0)
    assert np.all(np.abs(host - i3["relres"]) <= gap)


def test_a_column_does_not_depend_on_its_neighbours(cases, dcfm):
    shape = (60, 150, 5, 3)
    smp, _ = cases(shape)
    B = np.random.default_rng(12).standard_normal((shape[1], 40))
    X, info = smp.sigma_solve(B, tol=TOL, return_info=True)
    for j in (0, 7, 31, 32, 39):                                         # 32, 39: the second chunk
        xj, ij = smp.sigma_solve(B[:, j], tol=TOL, return_info=True)
        assert np.array_equal(xj, X[:, j]), j
        assert ij["relres"] == info["relres"][j] and ij["iters"] == info["iters"][j] and ij["quad"] == info["quad"][j]
    assert np.array_equal(smp.sigma_solve(B[:, 30:36], tol=TOL), X[:, 30:36])
    m2 = run_sampler(dcfm, shape, sigma_m2=True)
    try:
        assert np.array_equal(m2.sigma_solve(B, tol=TOL), X)             # the second moment changes nothing
    finally:
        m2.close()


def test_errors(cases, dcfm):
    from dcfm_amd import _abi
    smp, S = cases((60, 150, 5, 3))
    p = 150
    b = np.asfortranarray(np.random.default_rng(13).standard_normal((p, 1)))
    x, rel = np.full((p, 1), 7.0, order="F"), np.full(1, 7.0)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))                # noqa: E731
    fn = smp.lib.dcfm_sigma_solve
    bad = [(dp(b), 0, 1e-8, 10, dp(x), dp(rel)), (None, 1, 1e-8, 10, dp(x), dp(rel)),
           (dp(b), 1, 1e-8, 10, None, dp(rel)), (dp(b), 1, 1e-8, 10, dp(x), None),
           (dp(b), 1, 0.0, 10, dp(x), dp(rel)), (dp(b), 1, -1e-8, 10, dp(x), dp(rel)),
           (dp(b), 1, float("nan"), 10, dp(x), dp(rel)), (dp(b), 1, float("inf"), 10, dp(x), dp(rel)),
           (dp(b), 1, 1e-8, 0, dp(x), dp(rel))]
    for a in bad:
        assert fn(smp.h, *a, None, None, None) == _abi.DCFM_ERR_INVALID, a[1:4]
        assert np.all(x == 7.0) and np.all(rel == 7.0)                   # nothing written
    assert fn(smp.h, None, 1, 1e-8, 10, dp(x), dp(rel), None, None, None) == _abi.DCFM_ERR_INVALID
    assert b"null argument" in smp.lib.dcfm_last_error(smp.h)
    for badB in (np.zeros(p + 1), np.zeros((p - 1, 3)), np.zeros((p, 2, 2)), np.zeros(())):
        with pytest.raises(ValueError):
            smp.sigma_solve(badB)
    for kw in (dict(tol=0.0), dict(tol=-1.0), dict(max_iter=0)):
        with pytest.raises(dcfm.DcfmError) as e:
            smp.sigma_solve(b, **kw)
        assert e.value.code == _abi.DCFM_ERR_INVALID, kw
    # the handle still works, with the nullable outputs absent
    assert fn(smp.h, dp(b), 1, TOL, 300, dp(x), dp(rel), None, None, None) == _abi.DCFM_OK
    assert rel[0] <= TOL + 4.0 * 300 * p * EPS * kappa(S)
    assert np.array_equal(x, smp.sigma_solve(b, tol=TOL, max_iter=300))


def test_no_saved_sample_is_invalid(dcfm):
    from dcfm_amd import _abi
    c = make_case(40, 30, 3, 2, seed=21, k0=4)
    smp = dcfm.Sampler(c["n"], c["P"], 3, 2, c["rho"], 5, 4, 1, seed=7)
    try:
        smp.set_data(c["Yd"])
        smp.set_state({k: v for k, v in state_dict(c["st"]).items() if k != "eta"})
        smp.run(1, 3)                                                     # still inside the burn-in
        assert smp.saved_samples() == 0
        with pytest.raises(dcfm.DcfmError) as e:
            smp.sigma_solve(np.ones(30))
        assert e.value.code == _abi.DCFM_ERR_INVALID and "saved sample" in str(e.value)
        smp.run(4, 3)                                                     # past it: the handle still works
        assert smp.saved_samples() > 0
        x, info = smp.sigma_solve(np.ones(30), tol=TOL, return_info=True)
        assert info["converged"] and np.all(np.isfinite(x))
    finally:
        smp.close()


def test_loopback_ranks_return_the_same_bits(dcfm):
    p = 400
    B = np.random.default_rng(14).standard_normal((p, 40))

    def work(r, smp):
        S = smp.get_sigma()                                              # collective
        X, info = smp.sigma_solve(B, tol=TOL, return_info=True)
        x0 = smp.sigma_solve(B[:, 33], tol=TOL)
        return S, X, info, x0

    (S, X0, i0, a0), (_, X1, i1, a1) = loopback_pair(dcfm, work)
    assert np.array_equal(X0, X1) and np.array_equal(a0, a1)
    for f in ("relres", "iters", "quad"):
        assert np.array_equal(i0[f], i1[f]), f
    assert np.array_equal(a0, X0[:, 33])
    check_solution(S, B, X0, i0)


def test_driver_right_hand_sides(dcfm):
    import oracle
    n, p0, g, K = 40, 50, 4, 2
    Y, _ = oracle.synth.make_data(n, p0, k0=4, zero_cols=2)              # 48 kept columns
    B = np.random.default_rng(15).standard_normal((p0, 3))
    S, sol, info = dcfm.divideconquer(Y, g, K * g, 2, 6, 2, 0.5, seed=3, rhs=B, return_info=True)
    p = info["p"]                                                        # the solve's defaults: tol 1e-10
    assert p == 48 and set(sol) == {"x", "relres", "iters", "quad"} and sol["x"].shape == (p, 3)
    Bp = dcfm.permute_vectors(B, info["keep"], info["varind"])
    host = np.linalg.norm(Bp - S @ sol["x"], axis=0) / np.linalg.norm(Bp, axis=0)
    assert np.all(host <= 1e-10 + 4.0 * sol["iters"] * p * EPS * kappa(S))
    assert np.all(np.abs(sol["quad"] - np.sum(Bp * sol["x"], axis=0)) <= p * EPS * np.sum(np.abs(Bp * sol["x"]), axis=0))
    # with the components too: after their dict, before info; the default leaves the tuple as it was
    out = dcfm.divideconquer(Y, g, K * g, 2, 6, 2, 0.5, seed=3, n_components=2, rhs=B[:, 0], return_info=True)
    assert len(out) == 4 and "values" in out[1] and out[2]["x"].shape == (p,) and "varind" in out[3]
    host1 = np.linalg.norm(Bp[:, 0] - out[0] @ out[2]["x"]) / np.linalg.norm(Bp[:, 0])
    assert host1 <= 1e-10 + 4.0 * out[2]["iters"] * p * EPS * kappa(out[0])
    assert len(dcfm.divideconquer(Y, g, K * g, 2, 6, 2, 0.5, seed=3, return_info=True)) == 2
