"""The host Philox reference (oracle/philox_ref.py) is itself pinned, on the CPU:

  * Philox4x32-10 against the Random123 known-answer vectors;
  * the longdouble variates against an independent mpmath evaluation of the same formulas at 40
    digits, to 2^-60 relative -- three orders finer than anything tests/test_gpu_rng_exact.py asserts
    of the device (a few 2^-53);
  * the counter layout: every coordinate reaches the block, index pairs share one, the gamma and boost
    counters never collide;
  * the noise floor F_n of a plain double-precision Box-Muller, the unit the GPU bars are stated in.
"""
import mpmath
import numpy as np
import pytest

from philox_cases import GAMMA_AT, NORMAL_CASES, R, U, gamma_ref, noise_floor, normal_ref

LD = np.longdouble
REL = 2.0 ** -60

KAT = [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     "d16cfe09 94fdcceb 5001e420 24126ea1"),
]


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox4x32_10_known_answers(ctr, key, want):
    got = R.philox4x32_10(ctr, *key)
    assert " ".join(f"{int(v):08x}" for v in got) == want


def test_philox_is_vectorised_consistently():
    ctr = [np.array([c[0][i] for c in KAT], dtype=np.uint64) for i in range(4)]
    key = [np.array([c[1][i] for c in KAT], dtype=np.uint64) for i in range(2)]
    got = R.philox4x32_10(ctr, *key)
    for j, (_, _, want) in enumerate(KAT):
        assert " ".join(f"{int(v[j]):08x}" for v in got) == want


def test_u01_53_range_and_grid():
    assert float(R.u01_53(0, 0)) == U                       # smallest: 2^-53, never 0
    assert float(R.u01_53(0xFFFFFFFF, 0xFFFFFFFF)) == 1.0   # largest: exactly 1
    assert float(R.u01_53(0, 0x7FF)) == U                   # the low 11 bits are dropped
    assert float(R.u01_53(0, 0x800)) == 2 * U
    assert float(R.u01_53(0x80000000, 0)) == 0.5 + U


# ---- mpmath: the same formulas, written again on Python integers ----

def _mp_uniforms(seed, site, shard, row, x, it):
    r = [int(np.asarray(w).reshape(-1)[0]) for w in R.raw(seed, site, shard, row, x, it)]
    f = lambda hi, lo: mpmath.mpf((((hi << 32) | lo) >> 11) + 1) / mpmath.mpf(2) ** 53
    return f(r[0], r[1]), f(r[2], r[3])


def _mp_normal_pair(seed, site, shard, row, x, it):
    u1, u2 = _mp_uniforms(seed, site, shard, row, x, it)
    rad = mpmath.sqrt(-2 * mpmath.log(u1))
    return rad * mpmath.cos(2 * mpmath.pi * u2), rad * mpmath.sin(2 * mpmath.pi * u2)


def _mp_mt(shape, seed, site, shard, row, idx, it):
    d = mpmath.mpf(shape) - mpmath.mpf(1) / 3
    c = 1 / mpmath.sqrt(9 * d)
    for att in range(64):
        base = 0x80000000 | (idx << 8) | (att << 1)
        x = _mp_normal_pair(seed, site, shard, row, base, it)[0]
        v = 1 + c * x
        if v <= 0:
            continue
        v = v ** 3
        u = _mp_uniforms(seed, site, shard, row, base | 1, it)[0]
        if u < 1 - mpmath.mpf(0.0331) * x ** 4:
            return d * v, att
        if mpmath.log(u) < x * x / 2 + d * (1 - v + mpmath.log(v)):
            return d * v, att
    raise AssertionError("64 rejections")


def _mp_gamma(shape, seed, site, shard, row, idx, it):
    if shape in (1.0, 2.0):
        u1, u2 = _mp_uniforms(seed, site, shard, row, 0x80000000 | (idx << 8), it)
        return (-mpmath.log(u1) if shape == 1.0 else -mpmath.log(u1) - mpmath.log(u2)), 0
    if shape < 1.0:
        g1, att = _mp_mt(shape + 1.0, seed, site, shard, row, idx, it)
        U_ = _mp_uniforms(seed, site, shard, row, 0x80000000 | (idx << 8) | 0x80, it)[0]
        return g1 * mpmath.exp(mpmath.log(U_) / mpmath.mpf(shape)), att
    return _mp_mt(shape, seed, site, shard, row, idx, it)


def _to_mp(x):
    """A longdouble as an exact mpf (two doubles)."""
    hi = float(x)
    return mpmath.mpf(hi) + mpmath.mpf(float(LD(x) - LD(hi)))


def _assert_close(got_ld, want_mp, what):
    got = _to_mp(got_ld)
    if want_mp == 0:
        assert got == 0, what
    else:
        r = abs(got - want_mp) / abs(want_mp)
        assert r <= REL, f"{what}: relative error 2^{float(mpmath.log(r, 2)):.1f}"


def test_normals_match_mpmath_to_2pm60():
    """200 normals: the first 180 of the seed-123 fill, and from a scan of 2^20 counters the blocks with the
    smallest u1 and with u2 nearest each quadrant boundary (where a reference that rounded the angle
    2 pi u2 would lose its relative accuracy), both normals of each."""
    seed, site, shard, it, count = NORMAL_CASES["seed123"]
    ref = normal_ref("seed123")
    assert count == 1 << 20
    pick = list(range(180))
    pick += [int(np.argmin(ref.u1))]
    t = 4.0 * ref.u2
    dist = np.abs(t - np.rint(t))
    for q in range(4):                                       # nearest to 0 / 1, 1/4, 1/2, 3/4 of a turn
        d = np.where(np.rint(t).astype(int) % 4 == q, dist, np.inf)
        pick += [int(i) for i in np.argsort(d)[:2]]
    assert dist[pick[-1]] < 1e-4
    pick = sorted({i ^ b for i in pick for b in (0, 1)})[:200]
    with mpmath.workdps(40):
        for e in pick:
            row, idx = e // 32, e % 32
            got = R.normal(seed, site, shard, row, idx, it, extended=True)
            want = _mp_normal_pair(seed, site, shard, row, idx >> 1, it)[idx & 1]
            _assert_close(got.value, want, f"normal {e}")
            assert float(got.value) == ref.value[e]          # the fill is this value, rounded once


@pytest.mark.parametrize("shape", [2.0, 1.5, 501.0, 0.3])
def test_gammas_match_mpmath_to_2pm60(shape):
    """200 gammas per path (exponential, Marsaglia-Tsang small and large shape, boost), with the attempt
    that accepted; the variates with the most attempts and with the narrowest decisions are among them."""
    g = gamma_ref(shape)
    pick = set(range(190)) | {int(i) for i in np.argsort(g.margin)[:5]} | {int(i) for i in np.argsort(-g.attempt)[:5]}
    with mpmath.workdps(40):
        for e in sorted(pick):
            row, idx = e // 32, e % 32
            a = (GAMMA_AT["seed"], GAMMA_AT["site"], GAMMA_AT["shard"], row, idx, GAMMA_AT["iteration"])
            got = R.gamma(shape, *a, extended=True)
            want, att = _mp_gamma(shape, *a)
            assert int(got.attempt) == att, f"gamma {e}: attempt"
            _assert_close(got.value, want, f"gamma({shape}) {e}")
            assert float(got.value) == g.value[e]


# ---- counter layout ----

def _block(seed=5, site=3, shard=9, row=11, x=13, it=17):
    return tuple(int(np.asarray(w)) for w in R.raw(seed, site, shard, row, x, it))


def test_every_coordinate_reaches_the_block():
    base = _block()
    changed = dict(seed_low=_block(seed=6), seed_high=_block(seed=5 | (1 << 32)), site=_block(site=4),
                   shard=_block(shard=10), row=_block(row=12), pair=_block(x=14), iteration=_block(it=18),
                   shard_top_bit=_block(shard=9 | (1 << 23)), iteration_top_bit=_block(it=17 | (1 << 31)),
                   seed_top_bit=_block(seed=5 | (1 << 63)))
    for name, b in changed.items():
        assert b != base, name
    assert len(set(changed.values())) == len(changed)
    # site and shard are separate fields of one word: (site, shard) -> site << 24 | shard is one-to-one
    assert _block(site=3, shard=0xFFFFFF) != _block(site=4, shard=0)
    assert _block(site=1, shard=0) != _block(site=0, shard=1 << 23)
    # swapping two coordinates is not the same counter
    assert _block(row=13, x=11) != _block(row=11, x=13)
    assert _block(row=17, it=11) != _block(row=11, it=17)


def test_index_pairs_share_one_block():
    a = R.normal(7, 1, 2, 3, np.arange(0, 64, 2), 4)
    b = R.normal(7, 1, 2, 3, np.arange(1, 64, 2), 4)
    assert np.array_equal(a.u1, b.u1) and np.array_equal(a.u2, b.u2) and np.array_equal(a.rad, b.rad)
    assert not np.array_equal(a.value, b.value)
    np.testing.assert_allclose(a.value ** 2 + b.value ** 2, a.rad ** 2, rtol=8 * U)   # cos^2 + sin^2 = 1
    assert len(set(a.u1.tolist())) == 32                     # and different pairs do not


def test_gamma_and_boost_counters_are_distinct():
    i, a, b = np.meshgrid(np.arange(128), np.arange(64), np.arange(2), indexing="ij")
    gam = R.gamma_counter(i, a, b).ravel()
    boost = R.boost_counter(np.arange(128))
    allc = np.concatenate([gam, boost])
    assert len(set(allc.tolist())) == 128 * 64 * 2 + 128
    assert np.all(allc >> np.uint64(31) == 1) and np.all(allc < 1 << 32)   # never a normal's index >> 1
    assert int(R.gamma_counter(5, 3, 1)) == 0x80000000 | 5 << 8 | 3 << 1 | 1
    assert int(R.boost_counter(5)) == 0x80000000 | 5 << 8 | 0x80


def test_fill_is_row_major_over_width():
    for width in (1, 7, 32, 100):
        v = R.fill("normal", 3 * width + 2, 11, 1.0, 2, 3, 4, width=width)
        for e in (0, width - 1, width, 3 * width + 1):
            assert v[e] == R.normal(11, 2, 3, e // width, e % width, 4).value


# ---- the noise floor ----

def test_noise_floor_of_a_double_precision_box_muller():
    """F_n, the unit of the GPU bars (E <= 2 F_n).  Its a-priori ceiling: the unreduced angle fl(fl(2 pi) u2)
    is off by up to 4 u (half an ulp of a number in [4, 8)) + 2.2 u (fl(2 pi)'s own 0.35 u, times 2 pi);
    libm's cos / sin add <= 1 u, rad (log, product, sqrt) <= 2 u relative and the last product 0.5 u:
    F_n < 10 u whatever the libm.  A floor above that would mean the reference is off, not the naive form."""
    F = noise_floor()
    print(f"F_n = {F / U:.2f} u = {F:.3e}")
    assert 1.0 * U < F < 10.0 * U
