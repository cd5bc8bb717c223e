"""Host reference of the on-device Philox variates (TEST INFRASTRUCTURE ONLY — see oracle/__init__.py).

A plain NumPy restatement of what ``csrc/philox.h`` documents, written from that header's
comment and from Salmon et al., "Parallel random numbers: as easy as 1, 2, 3" (SC'11):

  * Philox4x32-10 on ``uint64`` arrays with 32-bit masking;
  * the counter layout  ctr = (x, row, site << 24 | shard, iteration),  key = (seed low, seed high),
    x = index >> 1 for normals (one block -> two Box-Muller normals) and
    x = 0x80000000 | index << 8 | attempt << 1 | bit for gammas (bit 0: the proposal's normal,
    bit 1: the acceptance uniform; 0x80 instead of attempt/bit: the uniform of the boost);
  * 53-bit uniforms in (0, 1] from word pairs (x, y) and (z, w);
  * Box-Muller, the Marsaglia-Tsang (2000) gamma, sums of exponentials for shapes 1 and 2 and the
    boost Ga(a) = Ga(a + 1) U^(1/a) for a < 1.

The device evaluates log, sqrt, sin and cos with short polynomial kernels in double precision; this
module does NOT restate those.  It evaluates the same formulas with ``np.log`` / ``np.sqrt`` /
``np.sin`` / ``np.cos`` in ``np.longdouble`` (x87 extended: 64-bit significand) and rounds to float64
once, at the end.  The angle 2 pi u is reduced exactly first (4u = q + f with q an integer and
|f| <= 1/2 is exact for a 53-bit u), so every variate keeps its RELATIVE accuracy next to a zero of
the sine or cosine; tests/test_philox_ref.py pins the result to mpmath at 40 digits.

Where ``np.longdouble`` is only a double the import fails with an AssertionError, and the tests that
need the reference skip with that reason instead of comparing at double precision.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from .draws import InitDraws, IterDraws, gamma_shapes

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, (
    f"np.longdouble has a {np.finfo(LD).nmant}-bit mantissa here; the Philox reference needs >= 63 bits")

M32 = np.uint64(0xFFFFFFFF)
SITES = dict(Z=1, X=2, LAMBDA=3, PSI=4, DELTA=5, PS=6, INIT_PS=7, INIT_X=8, INIT_PSI=9, INIT_Z=10,
             INIT_D1=11, INIT_D2=12, DIAG=15)
MAX_ATTEMPTS = 64                       # attempts occupy bits 1..6 of the gamma counter
GAMMA_BIT = 0x80000000
BOOST_BIT = 0x80

# pi/2 to 64 bits: the double nearest pi/2 plus the double nearest the remainder
HALF_PI = LD(1.57079632679489655800e+00) + LD(6.12323399573676603587e-17)

NormalDraw = namedtuple("NormalDraw", "value rad u1 u2")
GammaDraw = namedtuple("GammaDraw", "value attempt rad margin abs_log_u")


def _u64(a):
    return np.asarray(a, dtype=np.uint64)


def philox4x32_10(ctr4, k0, k1):
    """Philox4x32-10.  ctr4 = (x, y, z, w) and the key words broadcast; returns the four output words
    (x, y, z, w) as uint64 arrays holding 32-bit values."""
    M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    W0, W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
    s32 = np.uint64(32)
    x, y, z, w, k0, k1 = np.broadcast_arrays(*[_u64(v) & M32 for v in (*ctr4, k0, k1)])
    for _ in range(10):
        p0, p1 = M0 * x, M1 * z                     # 32 x 32 -> 64 bits: no overflow in uint64
        x, y, z, w = (p1 >> s32) ^ y ^ k0, p1 & M32, (p0 >> s32) ^ w ^ k1, p0 & M32
        k0, k1 = (k0 + W0) & M32, (k1 + W1) & M32
    return x, y, z, w


def u01_53(hi, lo):
    """53-bit uniform in (0, 1] from two 32-bit words, exact in longdouble."""
    v = (((_u64(hi) << np.uint64(32)) | _u64(lo)) >> np.uint64(11)) + np.uint64(1)
    return v.astype(LD) * LD(2.0) ** -53


def raw(seed, site, shard, row, x, it):
    """The Philox block at (site, shard, row, x, iteration) under the 64-bit seed."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    z = (_u64(site) << np.uint64(24)) | (_u64(shard) & np.uint64(0xFFFFFF))
    return philox4x32_10((_u64(x), _u64(row), z, _u64(int(it) & 0xFFFFFFFF)), seed & 0xFFFFFFFF, seed >> 32)


def _uniforms(seed, site, shard, row, x, it):
    r = raw(seed, site, shard, row, x, it)
    return u01_53(r[0], r[1]), u01_53(r[2], r[3])


def _sincos_turn(u):
    """(sin, cos) of 2 pi u for a 53-bit u in (0, 1], in longdouble, after the exact reduction
    4u = q + f, |f| <= 1/2."""
    t = LD(4.0) * u
    q = np.rint(t)
    ph = (t - q) * HALF_PI
    sp, cp = np.sin(ph), np.cos(ph)
    qi = q.astype(np.int64) & 3
    s = np.choose(qi, [sp, cp, -sp, -cp])
    c = np.choose(qi, [cp, -sp, -cp, sp])
    return s, c


def _box_muller(u1, u2):
    rad = np.sqrt(LD(-2.0) * np.log(u1))
    s, c = _sincos_turn(u2)
    return rad, rad * c, rad * s


def _out(extended):
    return (lambda a: np.asarray(a, dtype=LD)) if extended else (lambda a: np.asarray(a, dtype=np.float64))


def normal(seed, site, shard, row, idx, it, extended=False):
    """Standard normal ``idx`` of (site, shard, row, iteration): Box-Muller on block idx >> 1; even idx
    takes rad cos(2 pi u2), odd idx rad sin(2 pi u2).  Returns NormalDraw(value, rad, u1, u2), rounded to
    float64 unless ``extended``."""
    idx = _u64(idx)
    u1, u2 = _uniforms(seed, site, shard, row, idx >> np.uint64(1), it)
    rad, n0, n1 = _box_muller(u1, u2)
    v = np.where((idx & np.uint64(1)).astype(bool), n1, n0)
    f64 = _out(extended)
    return NormalDraw(f64(v), f64(rad), f64(u1), f64(u2))


def naive_normal_f64(seed, site, shard, row, idx, it):
    """The textbook Box-Muller in float64 NumPy (sqrt(-2 log u1) cos / sin (2 pi u2), no reduction), at the
    same counters.  Only used to measure the noise floor of a double-precision formulation."""
    idx = _u64(idx)
    u1, u2 = _uniforms(seed, site, shard, row, idx >> np.uint64(1), it)
    u1, u2 = u1.astype(np.float64), u2.astype(np.float64)
    rad, ang = np.sqrt(-2.0 * np.log(u1)), 2.0 * np.pi * u2
    return np.where((idx & np.uint64(1)).astype(bool), rad * np.sin(ang), rad * np.cos(ang))


def gamma_counter(idx, attempt, bit):
    """ctr.x of gamma ``idx``: attempt's normal block (bit 0) or acceptance uniform (bit 1)."""
    return (np.uint64(GAMMA_BIT) | ((_u64(idx) & np.uint64(0x7FFFFF)) << np.uint64(8))
            | (_u64(attempt) << np.uint64(1)) | _u64(bit))


def boost_counter(idx):
    return np.uint64(GAMMA_BIT) | ((_u64(idx) & np.uint64(0x7FFFFF)) << np.uint64(8)) | np.uint64(BOOST_BIT)


def _marsaglia_tsang(shape, seed, site, shard, row, idx, it):
    """Marsaglia & Tsang (2000), shape >= 1, one (base, base | 1) counter pair per attempt.  Returns
    longdouble value, accepting attempt, that attempt's rad, and the smallest |margin| of any comparison
    taken on the way (v > 0, the squeeze u < 1 - 0.0331 x^4, the log test)."""
    row, idx = np.broadcast_arrays(_u64(row), _u64(idx))
    shp = row.shape
    row, idx = row.ravel(), idx.ravel()
    N = idx.size
    d = LD(shape) - LD(1) / LD(3)
    c = LD(1) / np.sqrt(LD(9) * d)
    val = np.full(N, np.nan, dtype=LD)
    att_of = np.full(N, -1, dtype=np.int64)
    rad_of = np.full(N, np.nan, dtype=LD)
    margin = np.full(N, np.inf, dtype=LD)
    live = np.arange(N)
    for att in range(MAX_ATTEMPTS):
        if live.size == 0:
            break
        u1, u2 = _uniforms(seed, site, shard, row[live], gamma_counter(idx[live], att, 0), it)
        rad, x, _ = _box_muller(u1, u2)
        v1 = LD(1) + c * x
        margin[live] = np.minimum(margin[live], np.abs(v1))
        pos = v1 > 0
        v = v1 * v1 * v1
        u, _ = _uniforms(seed, site, shard, row[live], gamma_counter(idx[live], att, 1), it)
        x2 = x * x
        sq = u - (LD(1) - LD(0.0331) * x2 * x2)               # accept if < 0
        m = margin[live]
        margin[live] = np.where(pos, np.minimum(m, np.abs(sq)), m)
        acc = pos & (sq < 0)
        need_log = pos & ~acc
        with np.errstate(invalid="ignore", divide="ignore"):
            lt = np.log(u) - (LD(0.5) * x2 + d * (LD(1) - v + np.log(np.where(pos, v, LD(1)))))
        m = margin[live]
        margin[live] = np.where(need_log, np.minimum(m, np.abs(lt)), m)
        acc |= need_log & (lt < 0)
        a = live[acc]
        val[a], att_of[a], rad_of[a] = (d * v)[acc], att, rad[acc]
        live = live[~acc]
    assert live.size == 0, "a gamma was rejected 64 times: outside the device's counter scheme"
    return val.reshape(shp), att_of.reshape(shp), rad_of.reshape(shp), margin.reshape(shp)


def gamma(shape, seed, site, shard, row, idx, it, extended=False):
    """Standard gamma(shape) ``idx`` of (site, shard, row, iteration).  Returns GammaDraw: the value (float64),
    the attempt that accepted, that attempt's Box-Muller radius, the smallest absolute margin of any
    accept / reject comparison taken (inf where none is) and, for the boost, |log U| (else 0).  With
    ``extended`` the value stays in longdouble."""
    shape = float(shape)
    row, idx = np.broadcast_arrays(_u64(row), _u64(idx))
    f64, val = _out(False), _out(extended)
    zero = np.zeros(idx.shape)
    if shape == 1.0 or shape == 2.0:
        u1, u2 = _uniforms(seed, site, shard, row, gamma_counter(idx, 0, 0), it)
        v = -np.log(u1) if shape == 1.0 else -np.log(u1) - np.log(u2)
        return GammaDraw(val(v), zero.astype(np.int64), zero + np.nan, zero + np.inf, zero)
    if shape < 1.0:
        g1, att, rad, margin = _marsaglia_tsang(shape + 1.0, seed, site, shard, row, idx, it)
        U, _ = _uniforms(seed, site, shard, row, boost_counter(idx), it)
        lu = np.log(U)
        return GammaDraw(val(g1 * np.exp(lu / LD(shape))), att, f64(rad), f64(margin), f64(np.abs(lu)))
    v, att, rad, margin = _marsaglia_tsang(shape, seed, site, shard, row, idx, it)
    return GammaDraw(val(v), att, f64(rad), f64(margin), zero)


def fill(kind, count, seed=0, shape=1.0, site=15, shard=0, iteration=0, width=32, full=False):
    """Host twin of ``rng_fill`` / ``dcfm_rng_fill_rows``: variate e at row e // width, index e % width.
    Returns the float64 values, or with ``full`` the NormalDraw / GammaDraw they come in."""
    e = np.arange(int(count), dtype=np.uint64)
    row, idx = e // np.uint64(width), e % np.uint64(width)
    if kind == "normal":
        out = normal(seed, site, shard, row, idx, iteration)
    elif kind == "gamma":
        out = gamma(shape, seed, site, shard, row, idx, iteration)
    else:
        raise ValueError(kind)
    return out if full else out.value


class PhiloxSource:
    """The standard variates a generated-mode device chain consumes, in the layout of
    ``oracle.draws.DrawSource``: ``init()`` from sites 7-12 at iteration 0 (variate e = the column-major
    linear index inside the shard's array, row e // 32, index e % 32), ``iteration(it)`` from sites 1-6
    (row = i or j, index = k or h).  ``varind`` (dc:50) is not a device draw: pass it, or get the identity."""

    def __init__(self, seed, n, p, g, K, hyper, varind=None):
        if p % g:
            raise ValueError("p must be divisible by g (dc:41)")
        self.seed, self.n, self.p, self.g, self.K, self.P = int(seed), n, p, g, K, p // g
        self.hyper = hyper
        self.shapes = gamma_shapes(n, self.P, K, hyper)
        self.varind = np.arange(p) if varind is None else np.asarray(varind)

    def _linear(self, kind, site, m, rows, cols, shape=1.0):
        """rows x cols array whose column-major element e sits at (row e // 32, index e % 32)."""
        v = fill(kind, rows * cols, self.seed, shape, site, m, 0)
        return v.reshape(rows, cols, order="F")

    def _rows(self, kind, site, m, rows, width, it, shape=1.0):
        """rows x width array at (row, index)."""
        r, k = np.meshgrid(np.arange(rows), np.arange(width), indexing="ij")
        f = normal if kind == "normal" else (lambda *a: gamma(shape, *a))
        return f(self.seed, site, m, r, k, it).value

    def init(self) -> InitDraws:
        n, g, K, P, S, sh = self.n, self.g, self.K, self.P, SITES, self.shapes
        ps0 = np.stack([self._linear("gamma", S["INIT_PS"], m, P, 1, sh["ps0"]) for m in range(g)], axis=2)
        X0 = self._linear("normal", S["INIT_X"], 0, n, K)
        psi0 = np.stack([self._linear("gamma", S["INIT_PSI"], m, P, K, sh["psi0"]) for m in range(g)], axis=2)
        Z0 = np.stack([self._linear("normal", S["INIT_Z"], m, n, K) for m in range(g)], axis=2)
        delta0 = np.empty((K, g))
        for m in range(g):
            delta0[0, m] = fill("gamma", 1, self.seed, sh["delta0"][0], S["INIT_D1"], m, 0)[0]
            if K > 1:
                delta0[1:, m] = fill("gamma", K, self.seed, sh["delta0"][1], S["INIT_D2"], m, 0)[1:]
        return InitDraws(self.varind, ps0, X0, psi0, Z0, delta0)

    def iteration(self, it: int) -> IterDraws:
        n, g, K, P, S, sh = self.n, self.g, self.K, self.P, SITES, self.shapes
        NZ = np.stack([self._rows("normal", S["Z"], m, n, K, it).T for m in range(g)], axis=2)
        NX = self._rows("normal", S["X"], 0, n, K, it).T
        NL = np.stack([self._rows("normal", S["LAMBDA"], m, P, K, it).T for m in range(g)], axis=2)
        Gpsi = np.stack([self._rows("gamma", S["PSI"], m, P, K, it, sh["psi"]) for m in range(g)], axis=2)
        Gps = np.stack([self._rows("gamma", S["PS"], m, P, 1, it, sh["ps"])[:, 0] for m in range(g)], axis=1)
        Gdelta = np.empty((K, g))
        for m in range(g):
            for h in range(K):
                Gdelta[h, m] = gamma(sh["delta"][h], self.seed, S["DELTA"], m, 0, h, it).value
        return IterDraws(NZ, NX, NL, Gpsi, Gdelta, Gps)
