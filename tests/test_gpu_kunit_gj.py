"""Device primitives on their own (tests/kunit/kunit.hip), part 4: load_shifted, gj_invert and mat_apply of
csrc/gj.h (the K x K stages of the precision draws), 256 threads, one launch for every N and class.

A = I + 0.5 M is formed by load_shifted from M = 2 (F - I), F of family (a) or (c); 0.5 M is exact, so the
device's fma and the host's 0.5 M + I round once to the same matrix (checked bitwise), and that matrix is the
one the truth and the host references see.  The inverse is judged by max |A^ A - I| against numpy.linalg.inv
and the log det by its distance from the exact one against numpy.linalg.slogdet's, both under the 8x rule of
tests/kunit_ref.py with the floor 8 N 2^-53; mat_apply by the dot-product bound on the returned inverse.

The wrapper gives the global operands a pitch larger than their extent, as k_precision does (rows of M 131
apart, of the right-hand sides 35, of the product 37), so a stride taken for an extent shows.

Finding.  As first written gj_invert updated a pass's rows outside the pivot block as C (P^{-1} a), the panel
times the finished pivot rows.  That is the unblocked sweep's result in exact arithmetic only: it loses
cond(P) of the 4 x 4 pivot block, and every later pivot, the log det and the inverse were off by up to 1e5 x
the host's error (N = 5, cond 1e9) wherever a leading block is badly conditioned.  gj_invert now applies the
unblocked sweep's operations in their order (csrc/gj.h); kunit_ref.gj_blocked_ref restates it, and with
blk = 1 is the unblocked sweep itself, the second reference below."""
import functools

import numpy as np
import pytest

import kunit_ref as R

pytestmark = pytest.mark.gpu

NS = (1, 2, 3, 4, 5, 7, 8, 30, 32, 33, 63, 64, 65, 100, 127, 128)
NCOLS = (1, 15, 16, 17, 32)
KW, NC = 128, 32
LDM, LDR, LDP = 131, 35, 37       # kunit.hip GJ_LDM, GJ_LDR, GJ_LDP
CLASSES = ("a:1", "a:1000", "a:1e+06", "a:1e+09", "c:1", "c:100000")
BAD_N = 100


def _params():
    return [(N, c) for N in NS for c in CLASSES]


def _bad():
    ind = R.indefinite(R.fam_a(BAD_N, 1e3, 0), BAD_N // 2)
    zp = R.zero_pivot(R.fam_c(BAD_N, 1.0, 0), 37)
    return [ind, zp], [R.first_bad_pivot(ind), 37]


@functools.lru_cache(maxsize=None)
def _run():
    items = []
    for N in NS:
        cl = R.classes(N)
        for name in CLASSES:
            for A in cl[name]:
                items.append((N, name, A))
    for A in _bad()[0]:
        items.append((BAD_N, "bad", A))
    nm = len(items)
    rng = np.random.default_rng(21)
    M = np.full((nm, KW, LDM), np.nan)
    rhs = np.full((nm, KW, LDR), np.nan)
    ncs = np.array([NCOLS[m % len(NCOLS)] for m in range(nm)], dtype=np.int32)
    Ns = np.array([it[0] for it in items], dtype=np.int32)
    As, Bs = [], []
    for m, (N, _, F) in enumerate(items):
        Mm = 2.0 * (F - np.eye(N))
        As.append(0.5 * Mm + np.eye(N))
        Bs.append(rng.standard_normal((N, ncs[m])) * 10.0 ** rng.uniform(-3, 3, (N, ncs[m])))
        M[m, :N, :N] = Mm
        rhs[m, :N, :ncs[m]] = Bs[m]
    Aload = np.zeros((nm, KW * KW))
    Ainv = np.zeros((nm, KW * KW))
    logdet = np.zeros(nm)
    prod = np.full((nm, KW, LDP), 3.0)
    guard = np.zeros(nm, dtype=np.int32)
    assert R.lib().kunit_gj(R.ptr(M), R.ptr(Ns), R.ptr(ncs), nm, R.c_double(0.5), R.ptr(rhs), R.ptr(Aload), R.ptr(Ainv),
                            R.ptr(logdet), R.ptr(prod), R.ptr(guard)) == 0
    got = []
    for m, (N, _, _) in enumerate(items):
        got.append((Aload[m, :N * N].reshape(N, N), Ainv[m, :N * N].reshape(N, N), logdet[m],
                    prod[m, :N, :ncs[m]].copy(), np.concatenate([prod[m, :N, ncs[m]:].ravel(), prod[m, N:].ravel()])))
    return items, As, Bs, got, guard


def _class(N, cls):
    items, As, Bs, got, guard = _run()
    return [(A, B, g) for (n_, name, _), A, B, g in zip(items, As, Bs, got) if n_ == N and name == cls]


def test_guard_bands_and_load_shifted():
    items, As, Bs, got, guard = _run()
    assert guard.all(), "an LDS guard band was overwritten"
    for A, g in zip(As, got):
        assert np.array_equal(R.bits(g[0]), R.bits(A))


@pytest.mark.parametrize("N,cls", _params())
def test_gj_inverse(N, cls):
    e_dev = e_host = 0.0
    for A, _, (_, Ai, ld, _, _) in _class(N, cls):
        assert np.isfinite(Ai).all()
        e_dev = max(e_dev, R.inv_residual(Ai, A))
        e_host = max(e_host, R.inv_residual(np.linalg.inv(A), A))
    print(f"gj_invert N={N} {cls}: inverse dev {e_dev:.3e} host {e_host:.3e} ratio {e_dev / max(e_host, N * R.EPS53):.3g}")
    assert e_dev <= R.bar(e_host, N)


@pytest.mark.parametrize("N,cls", _params())
def test_gj_log_det(N, cls):
    l_dev = l_host = 0.0
    for A, _, (_, _, ld, _, _) in _class(N, cls):
        assert np.isfinite(ld)
        l_dev = max(l_dev, R.logdet_err(ld, A))
        l_host = max(l_host, R.logdet_err(np.linalg.slogdet(A)[1], A))
    print(f"gj_invert N={N} {cls}: log det dev {l_dev:.3e} host {l_host:.3e} ratio {l_dev / max(l_host, N * R.EPS53):.3g}")
    assert l_dev <= R.bar(l_host, N)


@pytest.mark.parametrize("N", NS)
def test_gj_invert_is_the_unblocked_sweep_and_mat_apply(N):
    """The blocked kernel against the unblocked pivot-free sweep (kunit_ref.gj_blocked_ref, blk = 1) under the same
    8x rule: a block update in another association shows here whatever LAPACK does.  And the product with the
    returned inverse is inside the dot-product bound."""
    worst, seen_nc, line = 0.0, set(), []
    for cls in CLASSES:
        e_dev = e_ref = l_dev = l_ref = 0.0
        for A, B, (_, Ai, ld, P, rest) in _class(N, cls):
            Ar, lr = R.gj_blocked_ref(A, blk=1)
            e_dev, e_ref = max(e_dev, R.inv_residual(Ai, A)), max(e_ref, R.inv_residual(Ar, A))
            l_dev, l_ref = max(l_dev, R.logdet_err(ld, A)), max(l_ref, R.logdet_err(lr, A))
            ex, zero_ok = R.dot_bound_excess(P, np.ascontiguousarray(Ai), np.ascontiguousarray(B.T))
            assert zero_ok and np.all(rest == 3.0)                         # nothing written past N x ncols
            worst = max(worst, ex)
            seen_nc.add(B.shape[1])
        line.append(f"{cls} {e_dev / max(e_ref, N * R.EPS53):.3g}/{l_dev / max(l_ref, N * R.EPS53):.3g}")
        assert e_dev <= R.bar(e_ref, N), (cls, e_dev, e_ref)
        assert l_dev <= R.bar(l_ref, N), (cls, l_dev, l_ref)
    print(f"gj_invert N={N}: dev / unblocked sweep (inverse/log det) " + "  ".join(line)
          + f";  mat_apply / bound {worst:.3f} (ncols {sorted(seen_nc)})")
    assert worst <= 1.0


def test_every_ncols_met_every_remainder():
    items, As, Bs, got, guard = _run()
    assert {B.shape[1] for B in Bs} == set(NCOLS)
    for nc in NCOLS:                                  # each panel width with small, odd and full N
        assert len({A.shape[0] for A, B in zip(As, Bs) if B.shape[1] == nc}) >= 8


def test_breakdown_gives_a_non_finite_log_det():
    items, As, Bs, got, guard = _run()
    mats, ks = _bad()
    d = R.ldl_pivots(As[-2])
    assert (d[:ks[0]] > 1e-6).all() and d[ks[0]] < -1e-6
    (_, Ai_neg, ld_neg, _, _), (_, Ai_zero, ld_zero, _, _) = got[-2], got[-1]
    assert not np.isfinite(ld_neg)                    # log of a negative pivot
    assert not np.isfinite(ld_zero) and not np.isfinite(Ai_zero).all()
    assert guard[-2] and guard[-1]
