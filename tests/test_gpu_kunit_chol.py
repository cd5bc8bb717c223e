"""Device primitives on their own (tests/kunit/kunit.hip), part 2: the one-wave Cholesky-and-inverse routines
chol_inv16_p, chol_inv16_blk and chol_inv32 (with mfma_tile32) of csrc/linalg.h on the matrix families of
tests/kunit_ref.py.  A returned U^ ~ L^{-1} is judged by E(U^) = max |U^ L* - I| against the exact factor,
relative to the same metric of the host's float64 factor-and-invert: per (routine, n, class),
max over seeds E_dev <= 8 x max over seeds E_host, floor 8 n 2^-53 (kunit_ref.bar).

What each routine reads, stated as the wrapper's row-major matrix S:
  chol_inv16_p<KP + 1, false>  the lower triangle (the strict upper is NaN here);
  chol_inv16_p<TLD, true>      a column-major tile read by rows, i.e. the upper triangle (strict lower NaN);
  chol_inv16_blk               the upper triangle (strict lower NaN);
  chol_inv32                   the lower triangle outside the (1, 1) block's strict upper part, which it reads
                               and rewrites but never consumes (NaN here too).
Breakdown (a non-positive pivot k).  chol_inv16_p eliminates in LDL' form: a negative pivot's reciprocal is
finite and only the closing 1 / sqrt(d_k) makes row k NaN, rows < k stay finite; a zero pivot's reciprocal is
not finite, the rows below it turn NaN at once and the finished rows of the same 16-block after them (their
multiplier 0 meets the NaN column in the fused multiply-add), so row k is NaN and only the rows of earlier
blocks are finite.  chol_inv16_blk takes the root of the pivot at once: rows < k finite, row k NaN, either way.

One case sits over the bar and is marked xfail(strict): chol_inv32 on the leading 16 x 16 block of
I + 1e5 G G' padded to 32, E_dev = 6.8e-13 against E_host = 4.9e-14 (ratio 13.9).  The routine returns
[U11 0; 0 I] with U11 bit for bit chol_inv16_p's result for the block (asserted below), and that result is
within the bar of the host's own factor-and-invert of the unpadded block (5.0e-13): LAPACK is ten times more
accurate on the padded matrix than on the block itself, the device is the same on both."""
import functools

import numpy as np
import pytest

import kunit_ref as R

pytestmark = pytest.mark.gpu

SEEDS = (0, 1)
NAN = np.nan


def _with_pads(n, pads):
    """classes(n) plus family (d): the leading N x N blocks of three of them."""
    cl = R.classes(n, SEEDS)
    for base in ("a:1000", "b:1e+06", "c:100000"):
        for N in pads:
            cl[f"d:{base}:N={N}"] = [R.fam_d(A, N) for A in cl[base]]
    return cl


def _flat(cl):
    names, mats = [], []
    for name, ms in cl.items():
        for A in ms:
            names.append(name)
            mats.append(A)
    return names, np.ascontiguousarray(np.array(mats))


def _canary(S, lower_read):
    S = S.copy()
    n = S.shape[-1]
    S[:, ~np.tri(n, dtype=bool) if lower_read else np.tri(n, k=-1, dtype=bool)] = NAN
    return np.ascontiguousarray(S)


def _names(n, pads):
    base = [f"{f}:{k:g}" for k in R.KAPPAS for f in "ab"] + ["c:1", "c:100000"]
    return base + [f"d:{b}:N={N}" for b in ("a:1000", "b:1e+06", "c:100000") for N in pads]


PADS16, PADS32 = (1, 5, 15), (1, 15, 16, 17, 31, 32)
NAMES16, NAMES32 = _names(16, PADS16), _names(32, PADS32)
XFAIL = {("chol_inv32", "d:c:100000:N=16"): "E_dev / E_host = 13.9: the host is 10x more accurate on the padded "
                                            "matrix than on the block; see the module docstring"}


def _params(routine, names):
    return [pytest.param(c, marks=pytest.mark.xfail(strict=True, reason=XFAIL[(routine, c)]))
            if (routine, c) in XFAIL else c for c in names]


@functools.lru_cache(maxsize=None)
def _cases(n):
    cl = _with_pads(n, PADS16 if n == 16 else PADS32)
    assert list(cl) == (NAMES16 if n == 16 else NAMES32)
    return _flat(cl)


def _errors(n, U, cls):
    """(E_dev, E_host) of class cls: each the max over its seeds"""
    names, mats = _cases(n)
    e_dev = e_host = 0.0
    for name, A, u in zip(names, mats, U):
        if name == cls:
            hi, lo = R.truth(A)[:2]
            e_dev = max(e_dev, R.E_metric(u, hi, lo))
            e_host = max(e_host, R.E_metric(R.host_uinv(A), hi, lo))
    return e_dev, e_host


def _judge(routine, n, U, cls):
    e_dev, e_host = _errors(n, U, cls)
    print(f"{routine} n={n} {cls}: E_dev {e_dev:.3e}  E_host {e_host:.3e}  ratio {e_dev / max(e_host, n * R.EPS53):.3g}")
    assert e_dev <= R.bar(e_host, n), (routine, cls, e_dev, e_host)


def _summary(routine, n, U):
    fam = {}
    for cls in (NAMES16 if n == 16 else NAMES32):
        e_dev, e_host = _errors(n, U, cls)
        fam[cls[0]] = max(fam.get(cls[0], 0.0), e_dev / max(e_host, n * R.EPS53))
    print(f"{routine} n={n}: worst E_dev / max(E_host, n 2^-53) per family: "
          + "  ".join(f"({k}) {v:.3g}" for k, v in sorted(fam.items())))


def _pads_are_identity(names, U):
    for name, u in zip(names, U):
        if name.startswith("d:"):
            N = int(name.split("N=")[1])
            n = u.shape[0]
            assert np.array_equal(u[N:, :], np.eye(n)[N:, :]) and not u[:N, N:].any(), name


# ---------------------------------------------------------------------------------------------- n = 16
@functools.lru_cache(maxsize=None)
def _run16p(variant, o):
    names, mats = _cases(16)
    S = _canary(mats, lower_read=(variant == 0))
    U = np.full_like(mats, 3.0)
    guard = np.zeros(len(mats), dtype=np.int32)
    assert R.lib().kunit_chol16p(R.ptr(S), len(mats), variant, o, R.ptr(U), R.ptr(guard)) == 0
    return U, guard


@functools.lru_cache(maxsize=None)
def _run16blk(hook):
    names, mats = _cases(16)
    S = _canary(mats, lower_read=False)
    U = np.full_like(mats, 3.0)
    H = np.full_like(mats, 3.0)
    assert R.lib().kunit_chol16blk(R.ptr(S), len(mats), hook, R.ptr(U), R.ptr(H)) == 0
    return U, H


VARIANTS = [(0, 0), (0, 16), (1, 0), (1, 16)]


def _p_name(variant, o):
    return f"chol_inv16_p<{'TLD, true' if variant else 'KP + 1, false'}> o={o}"


@pytest.mark.parametrize("variant,o", VARIANTS)
def test_chol_inv16_p_structure(variant, o):
    U, guard = _run16p(variant, o)
    assert guard.all(), "an LDS guard band was overwritten"
    assert np.isfinite(U).all()
    assert not U[:, ~np.tri(16, dtype=bool)].any(), "the triangle above the diagonal is not exactly 0"
    _pads_are_identity(_cases(16)[0], U)
    _summary(_p_name(variant, o), 16, U)


@pytest.mark.parametrize("cls", _params("chol_inv16_p", NAMES16))
@pytest.mark.parametrize("variant,o", VARIANTS)
def test_chol_inv16_p_accuracy(variant, o, cls):
    _judge(_p_name(variant, o), 16, _run16p(variant, o)[0], cls)


def test_chol_inv16_p_offsets_and_layouts_agree_bitwise():
    ref = R.bits(_run16p(0, 0)[0])
    for v in VARIANTS[1:]:
        assert np.array_equal(R.bits(_run16p(*v)[0]), ref), v


@pytest.mark.parametrize("hook", [0, 1])
def test_chol_inv16_blk_structure(hook):
    U, H = _run16blk(hook)
    assert np.isfinite(U).all()
    assert not U[:, ~np.tri(16, dtype=bool)].any()
    _pads_are_identity(_cases(16)[0], U)
    _summary(f"chol_inv16_blk hook={hook}", 16, U)
    if hook:   # the hook's own product came through: four block steps of A (16 x 4) B (4 x 16)
        i, k = np.arange(16)[:, None], np.arange(4)[None, :]
        Ah, Bh = (16 * k + i + 1).astype(float), (1.0 / (16 * k + i + 1)).T
        assert np.allclose(H, 4 * (Ah @ Bh), rtol=1e-14, atol=0)
    else:
        assert not H.any()


@pytest.mark.parametrize("cls", _params("chol_inv16_blk", NAMES16))
@pytest.mark.parametrize("hook", [0, 1])
def test_chol_inv16_blk_accuracy(hook, cls):
    _judge(f"chol_inv16_blk hook={hook}", 16, _run16blk(hook)[0], cls)


def test_chol_inv16_blk_hook_does_not_change_the_bits():
    assert np.array_equal(R.bits(_run16blk(0)[0]), R.bits(_run16blk(1)[0]))


# ---------------------------------------------------------------------------------------------- n = 32
@functools.lru_cache(maxsize=None)
def _run32():
    names, mats = _cases(32)
    S = _canary(mats, lower_read=True)
    B = np.ascontiguousarray(mats)
    U, T, M = (np.full_like(mats, 3.0) for _ in range(3))
    guard = np.zeros(len(mats), dtype=np.int32)
    assert R.lib().kunit_chol32(R.ptr(S), R.ptr(B), len(mats), R.ptr(U), R.ptr(T), R.ptr(M), R.ptr(guard)) == 0
    return U, T, M, guard


def test_chol_inv32_structure():
    U, T, M, guard = _run32()
    assert guard.all(), "an LDS guard band was overwritten"
    assert np.isfinite(U).all()
    assert not U[:, ~np.tri(32, dtype=bool)].any(), "the triangle above the diagonal is not exactly 0"
    _pads_are_identity(_cases(32)[0], U)
    _summary("chol_inv32", 32, U)


@pytest.mark.parametrize("cls", _params("chol_inv32", NAMES32))
def test_chol_inv32_accuracy(cls):
    _judge("chol_inv32", 32, _run32()[0], cls)


def test_chol_inv32_of_a_padded_block_is_chol_inv16_p_of_the_block():
    """N = 16: chol_inv32 returns [U11 0; 0 I], U11 bit for bit chol_inv16_p's, and U11 is within the bar of the
    host's factor-and-invert of the block itself (the ground of the one xfail above)."""
    names, mats = _cases(32)
    idx = [m for m, name in enumerate(names) if name.endswith("N=16")]
    blocks = np.ascontiguousarray(mats[idx][:, :16, :16])
    U16 = np.zeros_like(blocks)
    guard = np.zeros(len(idx), dtype=np.int32)
    assert R.lib().kunit_chol16p(R.ptr(_canary(blocks, True)), len(idx), 0, 0, R.ptr(U16), R.ptr(guard)) == 0
    U32 = _run32()[0][idx]
    assert np.array_equal(R.bits(U32[:, :16, :16]), R.bits(U16))
    e_dev, e_host = {}, {}
    for m, A, u in zip(idx, blocks, U16):
        hi, lo = R.truth(A)[:2]
        e_dev[names[m]] = max(e_dev.get(names[m], 0.0), R.E_metric(u, hi, lo))
        e_host[names[m]] = max(e_host.get(names[m], 0.0), R.E_metric(R.host_uinv(A), hi, lo))
    print({k: (e_dev[k], e_host[k]) for k in e_dev})
    for k in e_dev:
        assert e_dev[k] <= R.bar(e_host[k], 16), (k, e_dev[k], e_host[k])


def test_mfma_tile32_products():
    names, mats = _cases(32)
    U, T, M, guard = _run32()
    worst_t = worst_m = 0.0
    for A, u, t, m in zip(mats, U, T, M):
        ex, zero_ok = R.dot_bound_excess(t, u, u)                          # T = U U'   (NT)
        assert zero_ok
        worst_t = max(worst_t, ex)
        ex, zero_ok = R.dot_bound_excess(m, t, np.ascontiguousarray(A.T))  # M = T B    (NN)
        assert zero_ok
        worst_m = max(worst_m, ex)
    print(f"mfma_tile32: worst |C - X Y| / (33 2^-53 |X||Y|): NT {worst_t:.3f}  NN {worst_m:.3f}")
    assert worst_t <= 1.0 and worst_m <= 1.0


# ---------------------------------------------------------------------------------------------- breakdown
def _bad16():
    ind = R.indefinite(R.fam_a(16, 1e3, 0), 8)
    zp = R.zero_pivot(R.fam_c(16, 1.0, 0), 5)
    k = R.first_bad_pivot(ind)
    d = R.ldl_pivots(ind)
    assert 0 < k < 15 and (d[:k] > 1e-6).all() and d[k] < -1e-6            # float64 meets the same first bad pivot
    assert R.first_bad_pivot(zp) == 5
    return [ind, zp], [k, 5]


@pytest.mark.parametrize("variant", [0, 1])
def test_chol_inv16_p_breakdown(variant):
    mats, ks = _bad16()
    S = np.ascontiguousarray(np.array(mats))
    U = np.zeros_like(S)
    guard = np.zeros(2, dtype=np.int32)
    assert R.lib().kunit_chol16p(R.ptr(S), 2, variant, 0, R.ptr(U), R.ptr(guard)) == 0    # returns normally
    assert guard.all()
    assert np.isfinite(U[0][:ks[0]]).all() and not np.isfinite(U[0][ks[0], :ks[0] + 1]).any()   # negative pivot
    assert not np.isfinite(U[1][ks[1], :ks[1] + 1]).any()                                        # zero pivot


def test_chol_inv16_blk_breakdown():
    mats, ks = _bad16()
    S = np.ascontiguousarray(np.array(mats))
    U = np.zeros_like(S)
    H = np.zeros_like(S)
    assert R.lib().kunit_chol16blk(R.ptr(S), 2, 0, R.ptr(U), R.ptr(H)) == 0
    for u, k, w in zip(U, ks, ("indefinite", "zero pivot")):
        assert np.isfinite(u[:k]).all(), f"{w}: a row before pivot {k} is not finite"
        assert not np.isfinite(u[k, :k + 1]).any(), f"{w}: row {k} of the first non-positive pivot is finite"


@pytest.mark.parametrize("where", ["first block", "second block"])
def test_chol_inv32_breakdown(where):
    which, kz = (28, 7) if where == "first block" else (12, 21)
    ind = R.indefinite(R.fam_a(32, 1e3, 0), which)
    zp = R.zero_pivot(R.fam_c(32, 1.0, 0), kz)
    ks = [R.first_bad_pivot(ind), kz]
    assert (ks[0] < 16) == (where == "first block")
    d = R.ldl_pivots(ind)
    assert (d[:ks[0]] > 1e-6).all() and d[ks[0]] < -1e-6
    S = np.ascontiguousarray(np.array([ind, zp]))
    U, T, M = (np.zeros_like(S) for _ in range(3))
    guard = np.zeros(2, dtype=np.int32)
    assert R.lib().kunit_chol32(R.ptr(S), R.ptr(S), 2, R.ptr(U), R.ptr(T), R.ptr(M), R.ptr(guard)) == 0
    assert guard.all()
    for u, k, w in zip(U, ks, ("indefinite", "zero pivot")):
        lo = 16 * (k // 16)                  # chol_inv32 writes zeros right of a first-block row itself
        assert np.isfinite(u[:k if w == "indefinite" else lo]).all(), w
        assert not np.isfinite(u[k, lo:k + 1]).any(), w
