"""CPU checks of tests/kunit_ref.py: the truth, the metric's evaluation accuracy and sensitivity, the host
restatements of the device orders, and the inputs of the GPU unit tests (tests/test_gpu_kunit_*.py)."""
import math

import mpmath
import numpy as np
import pytest

import kunit_ref as R

TREE_NS = (1, 2, 3, 7, 8, 9, 63, 64, 65, 255, 256, 257, 1000)
DELTA_KS = (1, 2, 3, 31, 32, 33, 63, 64, 65, 100, 127, 128)


def test_families_are_what_they_say():
    for n in (16, 32, 100):
        for name, mats in R.classes(n).items():
            for A in mats:
                assert A.dtype == np.float64 and np.array_equal(A, A.T), name
                w = np.linalg.eigvalsh(A)
                assert w[0] > 0 or name.startswith("b:1e+09"), name       # (b) at 1e9 is singular to float64
        for k in R.KAPPAS:
            assert np.linalg.cond(R.fam_a(n, k, 0)) == pytest.approx(k, rel=1e-4)
    P = R.fam_d(R.fam_a(16, 1e3, 0), 5)
    assert np.array_equal(P[5:, 5:], np.eye(11)) and not P[5:, :5].any() and not P[:5, 5:].any()
    assert np.array_equal(P[:5, :5], R.fam_a(16, 1e3, 0)[:5, :5])


@pytest.mark.parametrize("n,make", [(16, lambda: R.fam_b(16, 1e9, 0)), (32, lambda: R.fam_a(32, 1e6, 1)),
                                    (33, lambda: R.fam_c(33, 1e5, 0))])
def test_fixed_point_truth_is_mpmath_cholesky(n, make):
    A = make()
    hi, lo, ld_hi, ld_lo = R.truth(A)
    with mpmath.workdps(60):
        L = mpmath.cholesky(mpmath.matrix(A.tolist()))
        worst = max(abs(mpmath.mpf(hi[i, j]) + mpmath.mpf(lo[i, j]) - L[i, j]) / abs(L[i, j])
                    for i in range(n) for j in range(i + 1))
        assert worst < mpmath.mpf(2) ** -104                               # hi + lo holds 106 bits
        rows = R.chol_fixed(A)
        exact = max(abs(mpmath.mpf(rows[i][j]) / mpmath.mpf(2) ** R.FRAC - L[i, j]) / abs(L[i, j])
                    for i in range(n) for j in range(i + 1))
        assert exact < mpmath.mpf(10) ** -45                               # the integers themselves: > 40 digits
        ld = 2 * mpmath.fsum(mpmath.log(L[i, i]) for i in range(n))
        assert abs(mpmath.mpf(ld_hi) + mpmath.mpf(ld_lo) - ld) < mpmath.mpf(10) ** -28
    assert not np.triu(hi, 1).any() and not np.triu(lo, 1).any()


def test_truth_rejects_a_non_positive_pivot():
    with pytest.raises(ArithmeticError):
        R.chol_fixed(R.indefinite(R.fam_a(16, 1e3, 0)))


def test_breakdown_inputs_break_where_they_say():
    for n, which in ((16, 8), (32, 28), (32, 12), (100, 50)):
        A = R.indefinite(R.fam_a(n, 1e3, 0), which)
        k = R.first_bad_pivot(A)
        d = R.ldl_pivots(A)
        assert 0 < k < n - 1 and (d[:k] > 1e-6).all() and d[k] < -1e-6     # float64 meets the exact first bad pivot
    for n, k in ((16, 5), (32, 7), (32, 21), (100, 37)):
        Z = R.zero_pivot(R.fam_c(n, 1.0, 0), k)
        assert R.first_bad_pivot(Z) == k and R.ldl_pivots(Z)[k] == 0.0 and (R.ldl_pivots(Z)[:k] > 0.5).all()
        assert np.array_equal(Z, Z.T)
    assert R.first_bad_pivot(R.fam_c(16, 1.0, 0)) is None


def test_gauss_jordan_restatement_inverts():
    for N in (1, 3, 4, 5, 7, 33, 100):
        for A in (R.fam_a(N, 1e3, 0), R.fam_c(N, 1.0, 1)):
            Ai, ld = R.gj_blocked_ref(A)
            assert R.inv_residual(Ai, A) < 1e3 * 1e3 * N * R.EPS53          # cond^2 n u: Gauss-Jordan's own bound
            assert np.allclose(Ai, np.linalg.inv(A), rtol=1e-9, atol=1e-12)
            assert R.logdet_err(ld, A) < 1e-11
            Ai1, ld1 = R.gj_blocked_ref(A, blk=1)                            # the unblocked sweep: the same operations
            assert ld1 == pytest.approx(ld, abs=1e-13) and np.allclose(Ai1, Ai, rtol=1e-12, atol=0)
    # the blocked order keeps the unblocked sweep's accuracy where a leading block is badly conditioned
    for N, A in ((5, R.fam_a(5, 1e9, 0)), (7, R.fam_a(7, 1e9, 1)), (100, R.fam_c(100, 1e5, 0))):
        e4, e1 = R.inv_residual(R.gj_blocked_ref(A)[0], A), R.inv_residual(R.gj_blocked_ref(A, blk=1)[0], A)
        assert e4 <= 2 * e1 and e1 <= 8 * max(R.inv_residual(np.linalg.inv(A), A), N * R.EPS53)


def test_fma_is_one_rounding():
    rng = np.random.default_rng(5)
    a = rng.standard_normal(400) * 10.0 ** rng.uniform(-20, 20, 400)
    b = rng.standard_normal(400) * 10.0 ** rng.uniform(-20, 20, 400)
    c = -a * b * (1 + rng.integers(-3, 4, 400) * 2.0 ** -52)               # heavy cancellation
    c[:100] = rng.standard_normal(100)
    with mpmath.workprec(53):
        for x, y, z in zip(a, b, c):
            p = mpmath.fmul(mpmath.mpf(float(x)), mpmath.mpf(float(y)), exact=True)
            want = mpmath.fadd(p, mpmath.mpf(float(z)), prec=53, rounding="n")
            assert mpmath.mpf(R.fma(x, y, z)) == want
    assert R.fma(2.0 ** -30, 2.0 ** -30, 1.0) == 1.0 and 2.0 ** -30 * 2.0 ** -30 + 1.0 == 1.0
    x = 1 + 2.0 ** -30
    assert R.fma(x, x, -1.0) != x * x - 1.0                                # the product's low bits survive


def test_metric_longdouble_agrees_with_mpmath_on_the_hardest_case():
    A = R.fam_b(128, 1e9, 0)
    hi, lo, _, _ = R.truth(A)
    U = R.host_uinv(A)
    e_host = R.E_metric(U, hi, lo)
    e_mp = R.E_metric_mp(U, A)
    print(f"E_host longdouble {e_host:.6e}  mpmath {e_mp:.6e}")
    assert abs(e_host - e_mp) <= 0.01 * e_host
    assert e_host > 128 * R.EPS53                                          # not an accidentally exact case


@pytest.mark.parametrize("n", [16, 32, 128])
@pytest.mark.parametrize("kappa", [1.0, 1e3])
def test_metric_flags_one_entry_off_by_1e_minus_12(n, kappa):
    for fam in (R.fam_a, R.fam_b):
        mats = [fam(n, kappa, s) for s in (0, 1)]
        e_host = max(R.E_metric(R.host_uinv(A), *R.truth(A)[:2]) for A in mats)
        A = mats[0]
        hi, lo = R.truth(A)[:2]
        U = R.host_uinv(A)
        e0 = R.E_metric(U, hi, lo)
        for (r, c) in ((n // 2, n // 2), (n - 1, n - 1), (0, 0)):             # U_rr L_rr = 1: the entry shows in full
            V = U.copy()
            V[r, c] *= 1 + 1e-12
            assert R.E_metric(V, hi, lo) > R.bar(e_host, n), (fam.__name__, r, c, e_host)
        # any entry (r, c): the metric moves by at least 1e-12 |U_rc| max_j |L*_cj|, less what was there before
        reach = np.abs(U) * np.abs(hi).max(axis=1)[None, :]
        r, c = np.unravel_index(np.argmax(reach - 2 * np.eye(n) * reach.max()), (n, n))
        assert r != c
        V = U.copy()
        V[r, c] *= 1 + 1e-12
        assert R.E_metric(V, hi, lo) >= 1e-12 * reach[r, c] * (1 - 1e-3) - e0


def test_host_references_are_finite_and_of_the_expected_size():
    """E_host, the residual of numpy's inverse and slogdet's error: finite on every class, not accidentally zero
    off cond 1, and (families (a) and (c), where cond is not a scaling's doing) below n eps cond(A)."""
    for n in (16, 32, 100):
        for name, mats in R.classes(n).items():
            for A in mats:
                e = R.E_metric(R.host_uinv(A), *R.truth(A)[:2])
                ri = R.inv_residual(np.linalg.inv(A), A)
                le = R.logdet_err(np.linalg.slogdet(A)[1], A)
                assert np.isfinite([e, ri, le]).all(), name
                if not name.endswith(":1"):
                    assert e > 0 and ri > 0
                if name[0] in "ac":
                    cond = np.linalg.cond(A)
                    assert e <= n * 2.0 ** -52 * cond and ri <= n * 2.0 ** -52 * cond, (name, e, ri, cond)
    # textbook scale of the metric at kappa = 1: a few n eps
    assert R.E_metric(R.host_uinv(R.fam_a(32, 1.0, 0)), *R.truth(R.fam_a(32, 1.0, 0))[:2]) < 32 * 2.0 ** -52


def _counter_tree(x):
    """TreeSum as linalg.h evaluates it: a binary counter of finished subtrees, totalled right to left."""
    s, i = {}, 0
    for v in x:
        v = np.float64(v)
        q = 0
        while (i >> q) & 1:
            v = s[q] + v
            q += 1
        s[q] = v
        i += 1
    acc = None
    for q in range(16):
        if (i >> q) & 1:
            acc = s[q] if acc is None else s[q] + acc
    return float(acc)


def test_tree_sum_reference_is_the_documented_tree():
    rng = np.random.default_rng(2)
    x = rng.standard_normal(1000) * 10.0 ** rng.uniform(-20, 20, 1000)
    f = np.float64
    assert R.tree_sum_ref(x[:3]) == (f(x[0]) + f(x[1])) + f(x[2])
    assert R.tree_sum_ref(x[:5]) == ((f(x[0]) + f(x[1])) + (f(x[2]) + f(x[3]))) + f(x[4])
    assert R.tree_sum_ref(x[:7]) == ((f(x[0]) + f(x[1])) + (f(x[2]) + f(x[3]))) + ((f(x[4]) + f(x[5])) + f(x[6]))
    for n in TREE_NS:
        t = R.tree_sum_ref(x[:n])
        assert t == _counter_tree(x[:n])
        assert abs(t - math.fsum(x[:n])) <= n * 2.0 ** -52 * np.abs(x[:n]).sum()
    # the order matters on these inputs
    assert len({R.tree_sum_ref(x[:257]), float(np.add.reduce(x[:257])), float(sum(x[:257]))}) > 1


def test_wave_order_references():
    src = R.lane_sources()
    assert src.shape == (R.LANE_ROWS, 64)
    for row in src[96 + 4:]:                                               # DPP permutes and the xor swaps
        assert sorted(row) == list(range(64))
    assert list(src[102][:16]) == [(i - 4) % 16 for i in range(16)] and src[102][16] == 28
    rng = np.random.default_rng(3)
    v = rng.standard_normal(64) * 10.0 ** rng.uniform(-20, 20, 64)
    rs = R.rowsum16_ref(v)
    for r in range(4):
        exact = math.fsum(v[16 * r:16 * r + 16])
        assert np.all(np.abs(rs[16 * r:16 * r + 16] - exact) <= 16 * 2.0 ** -52 * np.abs(v[16 * r:16 * r + 16]).sum())
    rs1 = R.rowsum16_ref(rng.standard_normal(64))                          # the lanes of a row do not agree
    assert any(len({float(t) for t in rs1[16 * r:16 * r + 16]}) > 1 for r in range(4))
    sp = R.scan_prod_ref(v)
    assert np.allclose(sp, np.cumprod(v), rtol=1e-13)
    ss = R.suffix_sum_ref(v)
    assert np.allclose(ss, np.cumsum(v[::-1])[::-1], rtol=0, atol=64 * 2.0 ** -52 * np.abs(v).sum())
    a = 10.0 ** rng.uniform(-2, 2, 64)
    b = 10.0 ** rng.uniform(-20, 20, 64)
    A, B = R.affine_scan_ref(a, b)
    y = 1.0
    for l in range(64):                                                    # the composed map applied to y_0 = 1
        y = a[l] * y + b[l]
        assert A[l] + B[l] == pytest.approx(y, rel=1e-12)


def test_delta_inputs_keep_the_serial_recurrence_finite():
    bd1, bd2 = 1.0, 2.5                                                    # test_gpu_kunit_delta.py BD1, BD2
    for K in DELTA_KS:
        for P in (20, 1250):
            for seed in (0, 1):
                t, G, io, ir = R.delta_inputs(K, P, seed)
                d = R.delta_serial(t, G, io, ir, bd1, bd2)
                assert np.all(np.isfinite(d)) and np.all(d > 0)
                assert 1e-3 <= (1 / io).min() and (1 / io).max() <= 1e3
    t, G, io, ir = R.delta_inputs(128, 1250, 0, underflow=True)
    d = R.delta_serial(t, G, io, ir, bd1, bd2)
    assert np.all(np.isfinite(d)) and np.all(d > 0)
    alpha = bd2 / (io * G)
    assert np.cumprod(alpha)[-1] == 0.0                                    # the running product of alpha underflows
    ref = R.delta_serial(t, G, io, ir, bd1, bd2, mp=True)
    assert R.rel_err_mp(d, ref) < 128 * 2.0 ** -48
