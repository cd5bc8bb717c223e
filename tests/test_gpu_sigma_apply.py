"""Y = Sigmaout V on the device (dcfm_sigma_apply, csrc/sigma_apply.hip) against the read-back matrix.

Shapes (n, p, g, K): the smallest that reach each branch of the kernel's tile walk --
(40, 30, 3, 2) one partial diagonal tile; (60, 150, 5, 3) two tile rows, a partial last tile,
P = 30 no multiple of 16; (60, 384, 4, 4) three exact tile rows; (60, 400, 4, 5) on two loopback
ranks, four tile rows split between them (by tile count: 3 + 1), so T0 > 0 on rank 1.

* Columns of the identity: every product is with 0 or 1 and every sum with zeros, so the result
  must be get_sigma_cols bit for bit (the mirror, the diagonal tile, the partial tiles).
* Random V: |Y - S V| <= 4 p eps (|S| |V|) componentwise -- gamma_p of a length-p dot product for
  each side's summation order, doubled; eps = 2^-52.
* The same input gives the same bytes; DCFM_FLAG_SIGMA_M2 changes nothing; two ranks return the
  same bytes.
"""
import ctypes as C

import numpy as np
import pytest

from sigma_cases import cases, loopback_pair, run_sampler  # noqa: F401  (cases: a fixture)

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
SHAPES = [(40, 30, 3, 2), (60, 150, 5, 3), (60, 384, 4, 4)]


def _bound(S, V, p):
    return 4.0 * p * EPS * (np.abs(S) @ np.abs(V))


def _starts(p, nv):
    """First columns: 0, across the 128 boundary (c0 = 120 with nv = 32 where p allows), the last ones."""
    out = {0, p - nv}
    if p >= 120 + nv:
        out.add(120)
    if p > 128:
        out.add(128 - nv // 2 if nv > 1 else 127)
    return sorted(c for c in out if 0 <= c <= p - nv)


@pytest.mark.parametrize("shape", SHAPES)
def test_identity_columns_are_sigma_columns_bit_for_bit(cases, shape):
    smp, S = cases(shape)
    p = shape[1]
    for nv in (1, 5, 32):
        if nv > p:
            continue
        for c0 in _starts(p, nv):
            V = np.zeros((p, nv))
            V[c0 + np.arange(nv), np.arange(nv)] = 1.0
            Y = smp.sigma_apply(V)
            ref = smp.get_sigma_cols(c0, nv)
            assert Y.shape == (p, nv)
            assert np.array_equal(Y, ref), (shape, nv, c0, float(np.max(np.abs(Y - ref))))
            assert np.array_equal(ref, S[:, c0:c0 + nv])


@pytest.mark.parametrize("shape", SHAPES)
def test_random_vectors_within_the_rounding_bound(cases, shape):
    smp, S = cases(shape)
    p = shape[1]
    rng = np.random.default_rng(5)
    for nv in (1, 5, 32, 40):                    # 40: two kernel passes inside the call
        V = rng.standard_normal((p, nv))
        Y = smp.sigma_apply(V)
        err, bd = np.abs(Y - S @ V), _bound(S, V, p)
        print(f"{shape} nv={nv}: max err / bound = {float(np.max(err / bd)):.3e}")
        assert np.all(err <= bd), (shape, nv, float(np.max(err / bd)))
        assert np.array_equal(smp.sigma_apply(V), Y), "same input, different bytes"


def test_shapes_and_device_time(cases):
    smp, S = cases((60, 150, 5, 3))
    p = 150
    v = np.random.default_rng(2).standard_normal(p)
    y, ms = smp.sigma_apply(v, return_ms=True)
    assert y.shape == (p,) and isinstance(ms, float) and ms > 0.0
    assert np.all(np.abs(y - S @ v) <= _bound(S, v[:, None], p)[:, 0])
    assert np.array_equal(smp.sigma_apply(v[:, None])[:, 0], y)
    Vc = np.ascontiguousarray(np.random.default_rng(3).standard_normal((p, 7)))    # C order in, same result
    assert np.array_equal(smp.sigma_apply(Vc), smp.sigma_apply(np.asfortranarray(Vc)))


def test_errors(cases, dcfm):
    from dcfm_amd import _abi
    smp, _ = cases((60, 150, 5, 3))
    p = 150
    buf = np.zeros((p, 1), order="F")
    dp = buf.ctypes.data_as(C.POINTER(C.c_double))
    assert smp.lib.dcfm_sigma_apply(smp.h, dp, 0, dp, None) == _abi.DCFM_ERR_INVALID
    assert smp.lib.dcfm_sigma_apply(smp.h, None, 1, dp, None) == _abi.DCFM_ERR_INVALID
    assert b"null argument" in smp.lib.dcfm_last_error(smp.h)
    for bad in (np.zeros(p + 1), np.zeros((p - 1, 3)), np.zeros((p, 2, 2)), np.zeros(())):
        with pytest.raises(ValueError):
            smp.sigma_apply(bad)
    assert np.array_equal(smp.sigma_apply(buf), buf)          # the handle still works; Sigma 0 = 0


def test_second_moment_flag_changes_nothing(cases, dcfm):
    shape = (60, 150, 5, 3)
    smp, _ = cases(shape)
    V = np.random.default_rng(9).standard_normal((shape[1], 5))
    m2 = run_sampler(dcfm, shape, sigma_m2=True)
    try:
        assert np.array_equal(m2.sigma_apply(V), smp.sigma_apply(V))
    finally:
        m2.close()


def test_loopback_ranks_agree(dcfm):
    p = 400
    rng = np.random.default_rng(4)
    V = rng.standard_normal((p, 40))
    E = np.zeros((p, 32))
    E[120 + np.arange(32), np.arange(32)] = 1.0               # across the 128 boundary and the ranks' split

    def work(r, smp):
        blk = smp.sigma_block()
        S = smp.get_sigma()                                   # collective
        return S, blk, smp.sigma_apply(V), smp.sigma_apply(E), smp.sigma_apply(V[:, 0])

    (S, b0, Y0, E0, y0), (_, b1, Y1, E1, y1) = loopback_pair(dcfm, work)
    # the four tile rows are split by tile count (6 + 4 tiles: rows 3 + 1), so T0 > 0 on rank 1
    assert b0["row0"] == 0 and b1["row0"] == b0["row1"] and 0 < b0["row1"] < p and b1["row1"] == p
    assert b0["row1"] % 128 == 0
    assert np.array_equal(Y0, Y1) and np.array_equal(E0, E1) and np.array_equal(y0, y1)
    assert np.all(np.abs(Y0 - S @ V) <= _bound(S, V, p))
    assert np.array_equal(E0, S[:, 120:152])
    assert np.array_equal(y0, Y0[:, 0])
