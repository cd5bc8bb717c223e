"""Device primitives on their own (tests/kunit/kunit.hip), part 1: the scalar reciprocals, the lane helpers,
the wave sums and scans, the canonical TreeSum and xcd_remap of csrc/linalg.h and affine_scan of csrc/delta.h.
The permutations and the summation orders are bitwise claims: each is compared, per lane, with the host
restatement of the documented order in tests/kunit_ref.py (checked on the CPU by tests/test_kunit_ref.py)."""
import ctypes

import mpmath
import numpy as np
import pytest

import kunit_ref as R

pytestmark = pytest.mark.gpu

TREE_NS = (1, 2, 3, 7, 8, 9, 63, 64, 65, 255, 256, 257, 1000)


def _scalar_args():
    rng = np.random.default_rng(11)
    x = 2.0 ** rng.uniform(-200.0, 200.0, 1 << 16)
    ulp = 2.0 ** -52
    edges = [1.0 - ulp / 2, 1.0, 1.0 + ulp, 2.0 - ulp, 2.0, 4.0 - 2 * ulp, 4.0]
    edges += [2.0 ** k for k in range(-200, 201)]                          # the powers of 2, those of 4 among them
    edges += [np.nextafter(2.0 ** k, 0.0) for k in range(-200, 201, 7)]
    edges += [np.nextafter(2.0 ** k, np.inf) for k in range(-200, 201, 7)]
    return np.concatenate([x, np.array(edges)])


BAD = np.array([0.0, -0.0, -1.0, -1e300, np.nan])


def test_scalar_reciprocals():
    x = _scalar_args()
    xs = np.ascontiguousarray(np.concatenate([x, BAD]))
    n = xs.size
    out = [np.full(n, 7.0) for _ in range(3)]
    assert R.lib().kunit_scalar(R.ptr(xs), n, *(R.ptr(o) for o in out)) == 0
    rsq, rsqh, rcp = out
    worst = [0.0, 0.0, 0.0]
    with mpmath.workprec(140):
        for i, v in enumerate(x):
            xv = mpmath.mpf(float(v))
            ir = 1 / mpmath.sqrt(xv)
            ic = 1 / xv
            worst[0] = max(worst[0], float(abs(mpmath.mpf(float(rsq[i])) - ir) / ir))
            worst[1] = max(worst[1], float(abs(mpmath.mpf(float(rsqh[i])) - ir) / ir))
            worst[2] = max(worst[2], float(abs(mpmath.mpf(float(rcp[i])) - ic) / ic))
    u = 2.0 ** -52
    print(f"max rel err / 2^-52: rsqrt_f64 {worst[0] / u:.3f}  rsqrt_f64_h {worst[1] / u:.3f}  rcp_f64 {worst[2] / u:.3f}")
    assert max(worst) <= u, worst
    k = x.size
    assert not np.isfinite(rsq[k:]).any() and not np.isfinite(rsqh[k:]).any()      # +0, -0, -1, -1e300, NaN
    assert not np.isfinite(rcp[k:k + 2]).any()                                        # rcp_f64(+-0)


def test_lane_helpers_are_exact_permutations():
    rng = np.random.default_rng(12)
    xb = rng.integers(0, 1 << 63, 64, dtype=np.uint64) * 2 + rng.integers(0, 2, 64, dtype=np.uint64)
    xb[5] = 0x8000000000000000                                             # -0
    xb[17] = 0x7FF8000000000123                                            # quiet NaN payloads
    xb[33] = 0xFFF8000000ABCDEF
    xb[48] = 0x7FF0000000000001                                            # a signalling NaN
    xb[63] = 0x0000000000000001                                            # the smallest subnormal
    assert len(set(xb.tolist())) == 64
    x = xb.view(np.float64)
    assert R.lib().kunit_lane_rows() == R.LANE_ROWS
    out = np.zeros((R.LANE_ROWS, 64))
    assert R.lib().kunit_lanes(R.ptr(x), R.ptr(out)) == 0
    want = xb[R.lane_sources()]
    bad = np.argwhere(out.view(np.uint64) != want)
    assert bad.size == 0, f"first wrong (row, lane): {bad[:8].tolist()}"


@pytest.fixture(scope="module")
def sums():
    rng = np.random.default_rng(13)
    nc = 8
    x = rng.choice([-1.0, 1.0], (nc, 64)) * 10.0 ** rng.uniform(-20.0, 20.0, (nc, 64))
    y = rng.choice([-1.0, 1.0], (nc, 64)) * 10.0 ** rng.uniform(-20.0, 20.0, (nc, 64))
    x[1] = np.abs(x[1])                                                    # the delta chain's case: all positive
    y[1] = np.abs(y[1])
    x[2] = 10.0 ** rng.uniform(-2.0, 2.0, 64)                              # the same magnitude: every add rounds
    out = [np.zeros((nc, 64)) for _ in range(5)]
    assert R.lib().kunit_sums(R.ptr(x), R.ptr(y), nc, *(R.ptr(o) for o in out)) == 0
    return x, y, out


def _same_bits(dev, ref, what):
    assert np.isfinite(ref).all(), what                                    # the order is only pinned on finite values
    bad = np.argwhere(R.bits(dev) != R.bits(ref))
    assert bad.size == 0, f"{what}: first wrong (case, lane) {bad[:8].tolist()}"


def test_rowsum16_order(sums):
    x, _, out = sums
    _same_bits(out[0], np.array([R.rowsum16_ref(v) for v in x]), "rowsum16")


def test_wave_scan_prod_and_suffix_sum_order(sums):
    x, _, out = sums
    with np.errstate(over="ignore", under="ignore"):
        ref = np.array([R.scan_prod_ref(v) for v in x])
    ok = np.isfinite(ref).all(axis=1)
    assert ok.sum() >= 4
    _same_bits(out[1][ok], ref[ok], "wave_scan_prod")
    _same_bits(out[2], np.array([R.suffix_sum_ref(v) for v in x]), "wave_suffix_sum")


def test_affine_scan_order(sums):
    x, y, out = sums
    with np.errstate(over="ignore", under="ignore"):
        ref = [R.affine_scan_ref(a, b) for a, b in zip(x, y)]
    A = np.array([r[0] for r in ref])
    B = np.array([r[1] for r in ref])
    ok = np.isfinite(A).all(axis=1) & np.isfinite(B).all(axis=1)
    assert ok.sum() >= 4 and ok[1] and ok[2]
    _same_bits(out[3][ok], A[ok], "affine_scan A")
    _same_bits(out[4][ok], B[ok], "affine_scan B")


def test_tree_sum_is_the_left_complete_tree():
    rng = np.random.default_rng(14)
    nsrc = 1000 * 33 + 7
    src = rng.choice([-1.0, 1.0], nsrc) * 10.0 ** rng.uniform(-20.0, 20.0, nsrc)
    cases = [(n, st, off) for n in TREE_NS for st, off in ((1, 0), (33, 0), (1, 5), (33, 7))]
    ns = np.array([c[0] for c in cases], dtype=np.int32)
    st = np.array([c[1] for c in cases], dtype=np.int32)
    off = np.array([c[2] for c in cases], dtype=np.int64)
    out = np.zeros((3, len(cases)))
    assert R.lib().kunit_tree(R.ptr(src), ctypes.c_longlong(nsrc), R.ptr(ns), R.ptr(st), R.ptr(off), len(cases),
                              R.ptr(out)) == 0
    ref = np.array([R.tree_sum_ref(src[o:o + (n - 1) * s + 1:s]) for n, s, o in cases])
    naive = np.array([float(np.cumsum(src[o:o + (n - 1) * s + 1:s])[-1]) for n, s, o in cases])
    assert (R.bits(ref) != R.bits(naive)).sum() >= len(cases) // 4        # the order shows on these inputs
    for k, name in enumerate(("tree_sum", "tree_sum_f<double, 4>", "TreeSum::push/total")):
        bad = np.argwhere(R.bits(out[k]) != R.bits(ref)).ravel()
        assert bad.size == 0, f"{name}: wrong for (n, stride, offset) {[cases[i] for i in bad[:6]]}"


def test_xcd_remap_is_a_bijection():
    totals = np.array([*range(1, 65), 255, 256, 257, 2496], dtype=np.int32)
    out = np.full(int(totals.sum()), -2, dtype=np.int32)
    assert R.lib().kunit_xcd(R.ptr(totals), totals.size, R.ptr(out)) == 0
    o = 0
    for t in totals:
        assert np.array_equal(np.sort(out[o:o + t]), np.arange(t)), f"total = {t}"
        o += t
