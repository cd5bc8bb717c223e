"""CPU tests of the missing-data feature's host side: the NumPy restatement of the imputation step against a naive
triple loop, the yy rule, the mask patterns, the driver's observed-entry standardisation against a per-column loop,
the mask's way through keep / varind, the output conversion and the ValueErrors -- all without a GPU."""
import numpy as np
import pytest

import missing_cases as mc


def _state(n, P, g, K, seed):
    r = np.random.default_rng(seed)
    return (r.standard_normal((n, P, g)), r.standard_normal((n, K, g)), r.standard_normal((P, K, g)),
            r.gamma(2.0, size=(P, 1, g)), r.standard_normal((n, P, g)))


@pytest.mark.parametrize("pattern", mc.PATTERNS)
def test_impute_ref_against_the_naive_loop(pattern):
    n, P, g, K = 13, 7, 3, 5
    Yd, eta, Lam, ps, z = _state(n, P, g, K, 1)
    mk = mc.make_mask(pattern, n, P, g)
    Y1, mu1 = mc.impute_ref(Yd, mk, eta, Lam, ps, z)
    Y2, mu2 = mc.impute_naive(Yd, mk, eta, Lam, ps, z)
    assert np.array_equal(Y1[~mk], Yd[~mk]) and np.array_equal(Y2[~mk], Yd[~mk])       # observed: untouched
    mag = mc.magnitude(mk, eta, Lam, ps, z)
    assert np.all(np.abs(Y1 - Y2)[mk] <= (K + 2) * 2.0 ** -53 * mag[mk])
    assert np.all(np.abs(mu1 - mu2) <= (K + 2) * 2.0 ** -53 * mag)
    if pattern == "none":
        assert np.array_equal(Y1, Yd)


def test_mask_patterns_hold_what_they_are_named_for():
    for (n, p, g, K), _ in mc.CASES.values():
        P = p // g
        rnd = mc.make_mask("random", n, P, g)
        assert 0.10 < rnd.mean() < 0.20
        ed = mc.make_mask("edges", n, P, g)
        assert ed[0, 0, 0] and ed[n - 1, P - 1, 0] and ed[5, :, 0].all()
        assert ed[:, 2, 0].sum() == n - 2 and not ed[:, :, g - 1].any()
        assert (ed.sum(axis=0) == 0).any()                                              # a column with none
        pr = mc.make_mask("pairs", n, P, g)
        assert pr[2, 0, 0] and pr[3, 0, 0] and pr[6, 0, 0] and not pr[7, 0, 0] and pr[9, 0, 0] and not pr[8, 0, 0]
        assert not mc.make_mask("none", n, P, g).any()


def test_yy_rule():
    n, P, g = 11, 5, 2
    Y = np.random.default_rng(2).standard_normal((n, P, g))
    mk = mc.make_mask("random", n, P, g, seed=3)
    yy = mc.yy_ref(Y, mk)
    for m in range(g):
        for j in range(P):
            so = sum(Y[i, j, m] ** 2 for i in range(n) if not mk[i, j, m])
            sm = sum(Y[i, j, m] ** 2 for i in range(n) if mk[i, j, m])
            assert yy[j, m] == pytest.approx(so + sm, rel=1e-15)
    assert np.allclose(yy, (Y * Y).sum(axis=0), rtol=1e-14)
    # rewriting is not incrementing: after many redraws the rule still gives the column's own sum
    for _ in range(50):
        Y = np.where(mk, np.random.default_rng(_).standard_normal(Y.shape), Y)
    assert np.allclose(mc.yy_ref(Y, mk), (Y * Y).sum(axis=0), rtol=1e-14)


def _holes(rng, n, p0, zero_col):
    Y = rng.standard_normal((n, p0)) * rng.uniform(0.5, 3.0, p0) + rng.uniform(-2, 2, p0)
    Y[:, zero_col] = 0.0
    Y[rng.random((n, p0)) < 0.2] = np.nan
    Y[:4, :] = np.where(np.isnan(Y[:4, :]), 1.0, Y[:4, :])     # every column keeps observed entries
    Y[:, zero_col] = np.where(np.isnan(Y[:, zero_col]), np.nan, 0.0)
    return Y


def test_observed_entry_standardisation_against_a_loop(dcfm):
    drv = dcfm.driver
    rng = np.random.default_rng(4)
    n, p0, g = 14, 9, 2
    Y = _holes(rng, n, p0, 3)
    Yk, n_, p, P, K, keep = drv.preprocess_missing(Y, g, 4)
    assert (n_, p, P, K) == (n, 8, 4, 2) and 3 not in keep                  # the zero-column scan ignores NaN
    assert np.array_equal(np.isnan(Yk), np.isnan(Y[:, keep]))
    varind = rng.permutation(p)
    Yd, mask = drv.partition_standardize_missing(Yk, g, varind)
    assert Yd.shape == mask.shape == (n, P, g) and mask.dtype == bool
    cols = drv.output_columns(keep, varind)
    for m in range(g):
        for j in range(P):
            c = Y[:, cols[m * P + j]]
            ob = ~np.isnan(c)
            assert np.array_equal(mask[:, j, m], ~ob)                       # the mask's way through keep / varind
            want = (c[ob] - c[ob].mean()) / c[ob].std(ddof=1)
            assert np.allclose(Yd[ob, j, m], want, rtol=1e-13, atol=1e-13)
            assert not Yd[~ob, j, m].any()                                  # missing entries are uploaded as 0
    mean, sd = drv.observed_moments(Y)
    assert np.allclose(mean[keep], np.nanmean(Y[:, keep], axis=0), rtol=1e-14)
    assert np.allclose(sd[keep], np.nanstd(Y[:, keep], axis=0, ddof=1), rtol=1e-14)
    assert mean[3] == 0.0 and sd[3] == 0.0
    # without holes it is dc:57-59 itself
    Yc = rng.standard_normal((n, 8))
    a, mk = drv.partition_standardize_missing(Yc, g, varind)
    assert not mk.any() and np.allclose(a, drv.partition_standardize(Yc, g, varind), rtol=1e-13, atol=1e-13)


def test_output_conversion(dcfm):
    drv = dcfm.driver
    rng = np.random.default_rng(5)
    n, p0, g = 14, 9, 2
    Y = _holes(rng, n, p0, 3)
    Yk, _, p, P, K, keep = drv.preprocess_missing(Y, g, 4)
    varind = rng.permutation(p)
    Yd, mask = drv.partition_standardize_missing(Yk, g, varind)
    mean, sd = drv.observed_moments(Y)
    imp = {"mean": np.where(mask, 0.25, Yd), "sd_total": np.where(mask, 2.0, 0.0), "mask": mask, "count": 7}
    out = drv.unstandardize_imputation(imp, Y, mean, sd, keep, varind)
    assert out["count"] == 7 and out["mean"].shape == out["sd"].shape == Y.shape
    ob = ~np.isnan(Y)
    assert np.array_equal(out["mean"][ob], Y[ob]) and not out["sd"][ob].any()
    assert not np.isnan(out["mean"]).any()
    hole = np.isnan(Y)
    hole[:, 3] = False
    want = np.broadcast_to(mean + 0.25 * sd, Y.shape)
    assert np.allclose(out["mean"][hole], want[hole], rtol=1e-14)
    assert np.allclose(out["sd"][hole], np.broadcast_to(2.0 * sd, Y.shape)[hole], rtol=1e-14)
    assert not out["mean"][:, 3].any() and not out["sd"][:, 3].any()       # the dropped column: 0 with sd 0
    # one rank of two fills in its own shard only
    half = {k: (v[:, :, 1:] if isinstance(v, np.ndarray) else v) for k, v in imp.items()}
    o1 = drv.unstandardize_imputation(half, Y, mean, sd, keep, varind, s0=1)
    c1 = drv.output_columns(keep, varind)[P:]
    assert np.array_equal(o1["mean"][:, c1], out["mean"][:, c1])
    c0 = drv.output_columns(keep, varind)[:P]
    assert np.array_equal(np.isnan(o1["mean"][:, c0]), np.isnan(Y[:, c0]))


def test_value_errors(dcfm):
    drv = dcfm.driver
    rng = np.random.default_rng(6)
    Y = rng.standard_normal((8, 4))
    Y[1:, 0] = np.nan                                                        # one observed entry
    with pytest.raises(ValueError, match="fewer than two"):
        drv.partition_standardize_missing(Y, 2, np.arange(4))
    Y = rng.standard_normal((8, 4))
    Y[:, 1] = np.where(np.arange(8) < 3, 2.5, np.nan)                         # constant where observed
    with pytest.raises(ValueError, match="zero variance"):
        drv.partition_standardize_missing(Y, 2, np.arange(4))
    with pytest.raises(ValueError, match="must be integers"):
        drv.preprocess_missing(rng.standard_normal((8, 5)), 2, 2)
    # impute with loglik is refused before anything is created (no GPU is touched)
    with pytest.raises(ValueError, match="loglik"):
        dcfm.divideconquer(rng.standard_normal((8, 4)), 2, 2, 1, 2, 1, 0.5, impute=True, loglik=True)
