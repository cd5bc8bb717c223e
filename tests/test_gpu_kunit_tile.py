"""Device primitives on their own (tests/kunit/kunit.hip), part 3: the tiled tile::potrf_inv + trtri + uut_store
of csrc/tile_linalg.h, staged as k_prep stages them, at TILE_THREADS = 1024 (the product's) and 128 (the
smallest the static_assert allows: one trailing wave beside wave 0's look-ahead).

Two launches (one per block size) run every N and class; the tests below read their share.  U^ = uout is
judged by E(U^) under the 8x rule of tests/kunit_ref.py; out against scale U^ U^' by the dot-product bound
(N + 1) 2^-53 |scale| (|U^||U^'|), the scale's own rounding inside it to first order."""
import numpy as np
import pytest

import kunit_ref as R

pytestmark = pytest.mark.gpu

NS = (33, 47, 48, 49, 64, 65, 100, 112, 113, 127, 128)
KW = 128
SCALE = 0.7071067811865476       # sqrt(1 - rho) at rho = 0.5
FILL = 3.0                       # what out and uout hold where the routines write nothing
CLASSES = ("a:1", "b:1", "a:1000", "b:1000", "a:1e+06", "b:1e+06", "a:1e+09", "b:1e+09", "c:1", "c:100000")
BAD_N = 100


def _bad():
    ind = R.indefinite(R.fam_a(BAD_N, 1e3, 0), BAD_N // 2)
    zp = R.zero_pivot(R.fam_c(BAD_N, 1.0, 0), 37)
    return [ind, zp], [R.first_bad_pivot(ind), 37]


@pytest.fixture(scope="module")
def runs():
    items = []                                   # (N, class, matrix)
    for N in NS:
        cl = R.classes(N)
        for name in CLASSES:
            for A in cl[name]:
                items.append((N, name, A))
    for A in _bad()[0]:
        items.append((BAD_N, "bad", A))
    S = np.zeros((len(items), KW, KW))
    for m, (N, _, A) in enumerate(items):
        S[m, :N, :N] = A
        S[m, N:, :] = np.nan                     # never read: the pad is formed in the kernel
        S[m, :, N:] = np.nan
    Ns = np.array([it[0] for it in items], dtype=np.int32)
    res = {}
    for threads in (1024, 128):
        out = np.full_like(S, FILL)
        uout = np.full_like(S, FILL)
        guard = np.zeros(len(items), dtype=np.int32)
        assert R.lib().kunit_tile(R.ptr(S), R.ptr(Ns), len(items), threads, R.c_double(SCALE), R.ptr(out), R.ptr(uout),
                                  R.ptr(guard)) == 0
        res[threads] = (out, uout, guard)
    return items, res


def test_block_sizes_agree_bitwise(runs):
    items, res = runs
    good = np.array([it[1] != "bad" for it in items])
    for k in (0, 1):
        assert np.array_equal(R.bits(res[1024][k][good]), R.bits(res[128][k][good]))
    assert res[1024][2].all() and res[128][2].all(), "an LDS guard band was overwritten"


@pytest.mark.parametrize("N", NS)
def test_potrf_inv_trtri_uut_store(runs, N):
    items, res = runs
    out, uout, guard = res[1024]
    nr = 16 * ((N + 15) // 16)
    e_dev, e_host, worst = {}, {}, 0.0
    for m, (n_, name, A) in enumerate(items):
        if n_ != N or name == "bad":
            continue
        U, T = uout[m], out[m]
        # the written region and nothing else
        assert np.all(U[nr:, :] == FILL) and np.all(U[:, nr:] == FILL) and np.all(T[nr:, :] == FILL) and np.all(T[:, nr:] == FILL)
        assert np.isfinite(U[:nr, :nr]).all() and np.isfinite(T[:nr, :nr]).all()
        assert not U[:nr, :nr][~np.tri(nr, dtype=bool)].any() and not U[N:nr, :nr].any(), name
        assert not T[N:nr, :nr].any() and not T[:nr, N:nr].any(), name
        assert np.array_equal(R.bits(T[:nr, :nr]), R.bits(T[:nr, :nr].T)), name
        Un = np.ascontiguousarray(U[:N, :N])
        hi, lo = R.truth(A)[:2]
        e_dev[name] = max(e_dev.get(name, 0.0), R.E_metric(Un, hi, lo))
        e_host[name] = max(e_host.get(name, 0.0), R.E_metric(R.host_uinv(A), hi, lo))
        ex, zero_ok = R.dot_bound_excess(T[:N, :N], Un, Un, SCALE)
        assert zero_ok
        worst = max(worst, ex)
    assert len(e_dev) == len(CLASSES)
    ratios = {name: e_dev[name] / max(e_host[name], N * R.EPS53) for name in e_dev}
    print(f"potrf_inv+trtri N={N}: E_dev / max(E_host, N 2^-53): "
          + "  ".join(f"{k} {v:.3g}" for k, v in ratios.items()) + f";  uut_store / bound {worst:.3f}")
    fails = [(name, e_dev[name], e_host[name]) for name in e_dev if not e_dev[name] <= R.bar(e_host[name], N)]
    assert not fails, f"(class, E_dev, E_host) over the bar: {fails}"
    assert worst <= 1.0


@pytest.mark.parametrize("threads", [1024, 128])
def test_breakdown_lands_in_the_pivot_row(runs, threads):
    items, res = runs
    out, uout, guard = res[threads]
    mats, ks = _bad()
    d = R.ldl_pivots(mats[0])
    assert (d[:ks[0]] > 1e-6).all() and d[ks[0]] < -1e-6
    idx = [m for m, it in enumerate(items) if it[1] == "bad"]
    for m, k, what in zip(idx, ks, ("indefinite", "zero pivot")):
        assert guard[m]
        U = uout[m]
        # a negative pivot's reciprocal is finite (LDL' form): rows < k stay finite; a zero pivot turns its whole
        # diagonal tile NaN (test_gpu_kunit_chol.py), so only the rows of earlier tiles are finite
        first = k if what == "indefinite" else 16 * (k // 16)
        assert np.isfinite(U[:first, :BAD_N]).all(), what
        assert not np.isfinite(U[k, :k + 1]).any(), what
        assert not np.isfinite(out[m][k, k]), what
