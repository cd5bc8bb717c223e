"""Host references, matrix families and metrics for the device-primitive unit tests
(tests/test_gpu_kunit_*.py, tests/kunit/kunit.hip); checked on the CPU by tests/test_kunit_ref.py.

Truth.  The Cholesky factor L* of a float64 matrix is computed in exact integer arithmetic on a fixed-point
grid of FRAC = 320 fractional bits (floor division and isqrt: every entry is within a few 2^-320 of the
exact factor of the exact input, ~90 digits for the entries here), because mpmath.cholesky costs a second
per 128 x 128 matrix and a golden file of hi + lo factors for every case would not fit a committed file.
test_kunit_ref.py checks it against mpmath at 60 digits.  L* is handed on as a float64 hi + lo pair.

Metric.  For a returned U^ ~ L^{-1}:  E(U^) = max |U^ L* - I|, evaluated in numpy.longdouble from hi + lo.
It is invariant under the scaling A -> D A D and its only cancellation is the truth's own.

Bar.  max over seeds of E_dev <= 8 x max over the same seeds of E_host, E_host the same metric for
scipy.linalg.solve_triangular(numpy.linalg.cholesky(A), I); floor 8 n 2^-53.
"""
from __future__ import annotations

import ctypes
import functools
import math
import operator
from fractions import Fraction
from pathlib import Path

import mpmath
import numpy as np
import scipy.linalg

EPS53 = 2.0 ** -53
FRAC = 320
LD = np.longdouble
KAPPAS = (1.0, 1e3, 1e6, 1e9)


# ------------------------------------------------------------------------------------------------ families
def _sym(A):
    A = np.tril(A) + np.tril(A, -1).T          # exactly symmetric: the lower triangle mirrored
    return np.ascontiguousarray(A, dtype=np.float64)


def fam_a(n, kappa, seed):
    """Q diag(s) Q', s log-spaced over 1 .. kappa."""
    rng = np.random.default_rng([seed, n, 1])
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    s = np.logspace(0.0, math.log10(kappa), n) if n > 1 else np.array([kappa])
    return _sym((Q * s) @ Q.T)


def fam_b(n, kappa, seed):
    """D A D, A of family (a), D log-spaced over 1 .. 1e6 (shuffled): ps E + diag(Plam) under the
    multiplicative-gamma prior."""
    rng = np.random.default_rng([seed, n, 2])
    d = np.logspace(0.0, 6.0, n) if n > 1 else np.array([1e3])
    d = rng.permutation(d)
    return _sym(fam_a(n, kappa, seed) * d[:, None] * d[None, :])


def fam_c(n, c, seed):
    """I + c G G', G n x max(n/2, 1): Zprec and B_m."""
    rng = np.random.default_rng([seed, n, 3])
    G = rng.standard_normal((n, max(n // 2, 1)))
    return _sym(np.eye(n) + c * (G @ G.T))


def fam_d(A, N):
    """The leading N x N block of A, identity beyond it."""
    P = np.eye(A.shape[0])
    P[:N, :N] = A[:N, :N]
    return P


def classes(n, seeds=(0, 1)):
    """{class name: [matrices over the seeds]}: families (a), (b) at the four kappa, (c) at c = 1, 1e5."""
    out = {}
    for k in KAPPAS:
        out[f"a:{k:g}"] = [fam_a(n, k, s) for s in seeds]
        out[f"b:{k:g}"] = [fam_b(n, k, s) for s in seeds]
    for c in (1.0, 1e5):
        out[f"c:{c:g}"] = [fam_c(n, c, s) for s in seeds]
    return out


def indefinite(A, which=0):
    """A with one eigenvalue (ascending index `which`) negated, the eigenvectors kept."""
    w, V = np.linalg.eigh(A)
    w[which] = -w[which]
    return _sym((V * w) @ V.T)


def ldl_pivots(A):
    """pivots d_k of the float64 elimination without pivoting (signs and sizes: a test's margin check)."""
    S = np.array(A, dtype=np.float64)
    d = np.zeros(S.shape[0])
    for k in range(S.shape[0]):
        d[k] = S[k, k]
        if d[k] == 0:
            d[k + 1:] = np.nan
            break
        S[k + 1:, k + 1:] -= np.outer(S[k + 1:, k], S[k, k + 1:]) / d[k]
    return d


def zero_pivot(A, k):
    """A with row and column k zeroed: l_kj = 0 for j < k whatever the rounding, so pivot k is exactly 0 in
    every elimination order, and the pivots before it are A's own."""
    B = A.copy()
    B[k, :] = 0.0
    B[:, k] = 0.0
    return B


def first_bad_pivot(A):
    """index of the first non-positive pivot of the exact elimination of A (None: positive definite)."""
    try:
        chol_fixed(A)
    except ArithmeticError as e:
        return e.pivot
    return None


# ------------------------------------------------------------------------------------------------ truth
def _fix(x):
    num, den = float(x).as_integer_ratio()           # den is a power of two
    return (num << FRAC) // den


def _unfix(v):
    """float64 hi + lo of the fixed-point integer v (int / int is correctly rounded)."""
    hi = v / (1 << FRAC)
    lo = (v - _fix(hi)) / (1 << FRAC)
    return hi, lo


def chol_fixed(A):
    """Rows of the lower Cholesky factor of the float64 matrix A (lower triangle read) as fixed-point
    integers; raises ArithmeticError on a non-positive pivot."""
    n = A.shape[0]
    rows = []
    for i in range(n):
        row = []
        for j in range(i + 1):
            s = (_fix(A[i, j]) << FRAC) - sum(map(operator.mul, row, rows[j] if j < i else row))
            if j < i:
                row.append(s // rows[j][j])
            else:
                if s <= 0:
                    err = ArithmeticError(f"pivot {i} is not positive")
                    err.pivot = i
                    raise err
                row.append(math.isqrt(s))
        rows.append(row)
    return rows


@functools.lru_cache(maxsize=None)
def _truth_cached(key, n):
    A = np.frombuffer(key, dtype=np.float64).reshape(n, n)
    rows = chol_fixed(A)
    hi = np.zeros((n, n))
    lo = np.zeros((n, n))
    for i, row in enumerate(rows):
        for j, v in enumerate(row):
            hi[i, j], lo[i, j] = _unfix(v)
    with mpmath.workprec(400):
        ld = 2 * mpmath.fsum(mpmath.log(mpmath.mpf(rows[i][i]) / mpmath.mpf(2) ** FRAC) for i in range(n))
        ld_hi = float(ld)
        ld_lo = float(ld - mpmath.mpf(ld_hi))
    return hi, lo, ld_hi, ld_lo


def truth(A):
    """(L* hi, L* lo, log det hi, log det lo) of the float64 SPD matrix A."""
    A = np.ascontiguousarray(A, dtype=np.float64)
    return _truth_cached(A.tobytes(), A.shape[0])


# ------------------------------------------------------------------------------------------------ metrics
def E_metric(U, Lhi, Llo):
    """max |U L* - I| in longdouble."""
    U = np.asarray(U, dtype=np.float64).astype(LD)
    R = U @ Lhi.astype(LD) + U @ Llo.astype(LD) - np.eye(U.shape[0], dtype=LD)
    return float(np.max(np.abs(R)))


def E_metric_mp(U, A, dps=60):
    """The same, all in mpmath (its own Cholesky of A): the check of E_metric."""
    n = A.shape[0]
    with mpmath.workdps(dps):
        L = mpmath.cholesky(mpmath.matrix(A.tolist()))
        Lc = [[L[k, j] for k in range(n)] for j in range(n)]
        worst = mpmath.mpf(0)
        for i in range(n):
            ui = [mpmath.mpf(float(U[i, k])) for k in range(n)]
            nz = np.nonzero(U[i])[0]
            kend = int(nz.max()) + 1 if nz.size else 0
            for j in range(n):                # L*[k][j] = 0 for k < j, U[i][k] = 0 for k >= kend
                r = mpmath.fdot(ui[j:kend], Lc[j][j:kend]) - (1 if i == j else 0)
                worst = max(worst, abs(r))
        return float(worst)


def host_uinv(A):
    return scipy.linalg.solve_triangular(np.linalg.cholesky(A), np.eye(A.shape[0]), lower=True)


def inv_residual(Ai, A):
    """max |Ai A - I| in longdouble."""
    R = np.asarray(Ai, dtype=np.float64).astype(LD) @ A.astype(LD) - np.eye(A.shape[0], dtype=LD)
    return float(np.max(np.abs(R)))


def logdet_err(ld, A):
    _, _, hi, lo = truth(A)
    return float(abs((LD(ld) - LD(hi)) - LD(lo)))


def bar(e_host, n):
    """The 8x rule with its floor."""
    return 8.0 * max(float(e_host), n * EPS53)


def dot_bound_excess(C, X, Y, scale=1.0):
    """max of |C - scale X Y'| / ((n + 1) 2^-53 |scale| |X||Y'|) over the entries with a non-zero bound (<= 1
    passes: the dot-product bound, n = the inner length), and whether C is exactly 0 wherever the bound is.
    X, Y float64; the product in longdouble."""
    n = X.shape[1]
    Xl, Yl = X.astype(LD), Y.astype(LD)
    P = scale * (Xl @ Yl.T)
    Bd = (n + 1) * EPS53 * abs(scale) * (np.abs(Xl) @ np.abs(Yl).T)
    D = np.abs(np.asarray(C, dtype=np.float64).astype(LD) - P)
    nz = Bd > 0
    zero_ok = bool(np.all(np.asarray(C)[~nz] == 0.0))
    return (float(np.max(D[nz] / Bd[nz])) if nz.any() else 0.0), zero_ok


def gj_blocked_ref(A, blk=4):
    """csrc/gj.h's gj_invert restated in plain float64 NumPy (no fused multiply-add, whole-matrix updates): the
    pivot-free Gauss-Jordan inverse, `blk` pivots a pass, every row updated in the order of the unblocked sweep.
    The pivot rows (the block's columns as unit vectors) run through the block's eliminations; U_q is pivot
    row q as it stands when pivot q is taken and S_q its entries in the block's later columns.  A row outside
    the block takes its multipliers m_q = C_q - sum_{q' < q} m_q' S_q'[q] and then A(i, :) -= sum_q m_q U_q.
    blk = 1 is the unblocked sweep itself.  Returns (inverse, log det)."""
    A = np.array(A, dtype=np.float64)
    N = A.shape[0]
    lg = 0.0
    for kb in range(0, N, blk):
        b = list(range(kb, min(kb + blk, N)))
        bs = len(b)
        P = A[np.ix_(b, b)].copy()
        R_ = A[b, :].copy()
        R_[:, b] = np.eye(bs)
        M = A[:, b].copy()
        M[b, :] = 0.0
        V = A.copy()
        V[:, b] = 0.0
        for q in range(bs):
            lg += float(np.log(P[q, q])) if P[q, q] > 0 else float("nan")
            ip = 1.0 / P[q, q]
            rq = P[q].copy()
            rq[q] = 1.0
            rq *= ip
            aq = R_[q] * ip
            for r in range(bs):
                if r != q:
                    f = P[r, q]
                    row = P[r].copy()
                    row[q] = 0.0
                    P[r] = row - f * rq
                    R_[r] = R_[r] - f * aq
            P[q] = rq
            R_[q] = aq
            for c in range(q + 1, bs):                 # the later multipliers of the rows outside the block
                M[:, c] = M[:, c] - M[:, q] * rq[c]
            V = V - np.outer(M[:, q], aq)
        V[b, :] = R_
        A = V
    return A, lg


# ------------------------------------------------------------------------------------------------ exact fma
def fma(a, b, c):
    """round(a b + c) to float64 with one rounding: exact rationals, and int / int is correctly rounded
    (test_kunit_ref.py checks it against mpmath's exact product and sum)."""
    return float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


# ------------------------------------------------------------------------------------------------ wave order
def _dpp_src(ctrl):
    """source lane of every lane of a wave for the DPP controls of rowsum16."""
    l = np.arange(64)
    if ctrl < 0x100:                                           # quad_perm
        sel = np.array([(ctrl >> (2 * i)) & 3 for i in range(4)])
        return (l & ~3) + sel[l & 3]
    assert 0x121 <= ctrl <= 0x12F                              # row_ror:n: lane i takes lane (i - n) mod 16
    return (l & ~15) + ((l & 15) - (ctrl & 15)) % 16


LANE_ROWS = 106


def lane_sources():
    """source lane of every lane for the LANE_ROWS rows of kunit_lanes."""
    l = np.arange(64)
    rows = [np.full(64, s) for s in range(64)]
    rows += [np.where(l >= 32, 32 + c, c) for c in range(32)]
    rows += [(l & ~3) + j for j in range(4)]
    rows += [_dpp_src(c) for c in (0xB1, 0x4E, 0x124, 0x128)]
    rows += [l ^ 16, l ^ 32]
    return np.array(rows)


def rowsum16_ref(v):
    v = np.array(v, dtype=np.float64)
    for ctrl in (0xB1, 0x4E, 0x124, 0x128):
        v = v + v[_dpp_src(ctrl)]
    return v


def scan_prod_ref(v):
    v = np.array(v, dtype=np.float64)
    l = np.arange(64)
    o = 1
    while o < 64:
        u = v[np.maximum(l - o, 0)]
        v = np.where(l >= o, v * u, v)
        o <<= 1
    return v


def suffix_sum_ref(v):
    v = np.array(v, dtype=np.float64)
    l = np.arange(64)
    o = 1
    while o < 64:
        u = v[np.minimum(l + o, 63)]
        v = np.where(l + o < 64, v + u, v)
        o <<= 1
    return v


def affine_scan_ref(A, B):
    A = np.array(A, dtype=np.float64)
    B = np.array(B, dtype=np.float64)
    o = 1
    while o < 64:
        An, Bn = A.copy(), B.copy()
        for l in range(o, 64):
            Bn[l] = fma(A[l], B[l - o], B[l])
            An[l] = A[l] * A[l - o]
        A, B = An, Bn
        o <<= 1
    return A, B


def tree_sum_ref(x):
    """T(0, n) = T(0, h) + T(h, n - h), h the largest power of two below n."""
    x = [float(v) for v in x]

    def T(a, n):
        if n == 1:
            return x[a]
        h = 1 << ((n - 1).bit_length() - 1)
        return float(np.float64(T(a, h)) + np.float64(T(a + h, n - h)))
    return T(0, len(x))


# ------------------------------------------------------------------------------------------------ delta chain
def delta_inputs(K, P, seed, ad=2.0, underflow=False):
    """t_h = tau_h s_h, G_h ~ Gamma(ad + P (K - h) / 2), delta_old over 1e-3 .. 1e3 and a reference delta
    (1 / delta_ref enters c_h), all float64 of length K.  underflow: alpha_h = b_h dold_h / G_h ~ 1e-3 .. 1e-6
    every step, so that the running product of alpha leaves the float64 range within K = 128."""
    rng = np.random.default_rng([seed, K, P])
    h = np.arange(K)
    G = rng.gamma(ad + 0.5 * P * (K - h))
    dold = 10.0 ** rng.uniform(-3.0, 3.0, K)
    dref = 10.0 ** rng.uniform(-3.0, 3.0, K)
    if underflow:
        dold = 10.0 ** rng.uniform(-3.0, -1.0, K)
        G = G + 1e3
    t = rng.gamma(0.5 * P, 2.0, K) * 10.0 ** rng.uniform(-1.0, 1.0, K)      # tau_h s_h ~ a chi-square of P
    return t, G, 1.0 / dold, 1.0 / dref


def delta_serial(t, G, idold, idref, bd1, bd2, mp=False):
    """The K-step chain of delta.h's header: T_h = sum_{l >= h} t_l, bd_h = b_h + (0.5 / dref_h) F_h T_h,
    dn_h = G_h / bd_h, F_{h+1} = F_h dn_h / dold_h.  mp: in mpmath at 60 digits (float64 inputs exact);
    else plain float64, serially."""
    K = len(t)
    if mp:
        with mpmath.workdps(60):
            c = [mpmath.mpf(float(v)) for v in t]
            T = [mpmath.fsum(c[h:]) for h in range(K)]
            F = mpmath.mpf(1)
            out = []
            for h in range(K):
                bd = (bd1 if h == 0 else bd2) + mpmath.mpf(0.5) * mpmath.mpf(float(idref[h])) * F * T[h]
                dn = mpmath.mpf(float(G[h])) / bd
                F = F * dn * mpmath.mpf(float(idold[h]))
                out.append(dn)
            return out
    T = np.zeros(K)
    acc = 0.0
    for h in range(K - 1, -1, -1):
        acc = acc + t[h]
        T[h] = acc
    F = 1.0
    out = np.zeros(K)
    for h in range(K):
        bd = (bd1 if h == 0 else bd2) + (0.5 * idref[h]) * (F * T[h])
        out[h] = G[h] / bd
        F = F * out[h] * idold[h]
    return out


def rel_err_mp(x, ref):
    with mpmath.workdps(60):
        return float(max(abs(mpmath.mpf(float(a)) - r) / abs(r) for a, r in zip(x, ref)))


# ------------------------------------------------------------------------------------------------ library
LIB_PATH = Path(__file__).resolve().parent / "kunit" / "libdcfm_kunit.so"


@functools.lru_cache(maxsize=None)
def lib():
    """libdcfm_kunit.so (built by csrc/Makefile's default target); a missing library is an error."""
    L = ctypes.CDLL(str(LIB_PATH))
    for name in ("scalar", "lane_rows", "lanes", "sums", "tree", "xcd", "chol16p", "chol16blk", "chol32", "tile", "gj",
                 "delta", "slot"):
        getattr(L, "kunit_" + name).restype = ctypes.c_int
    return L


c_double = ctypes.c_double


def ptr(a):
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(ctypes.c_void_p)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


SENTINEL = np.array([0x7FF8DCF0BADC0DE5], dtype=np.uint64).view(np.float64)[0]
