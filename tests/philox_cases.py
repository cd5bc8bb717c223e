"""Shared by tests/test_philox_ref.py (CPU) and tests/test_gpu_rng_exact.py (GPU): the fixed counters of the
exact RNG comparison, the host reference at those counters (computed once per session, never modified)
and the noise floor F_n the GPU bars are stated in."""
from __future__ import annotations

import functools

import numpy as np
import pytest

try:
    from oracle import philox_ref as R
except AssertionError as exc:           # np.longdouble is a plain double on this platform
    pytest.skip(str(exc), allow_module_level=True)

U = 2.0 ** -53                          # unit roundoff of float64

SEED64 = 0x9E3779B97F4A7C15
# (seed, site, shard, iteration, count).  The first is the statistical test's counter set; 2^20 variates
# of it (the 2^18 of the second, and more) because its 2^18 smallest u1 is only 2^-16: the fill has to
# reach u1 < 2^-20 (2^-22.9 at variates 2^18 .. 2^20), the far tail of the device's log.
NORMAL_CASES = {
    "seed123": (123, 1, 5, 7, 1 << 20),
    "seed64bit": (SEED64, 1, 5, 7, 1 << 18),
}
GAMMA_AT = dict(seed=99, site=4, shard=2, iteration=3)
GAMMA_COUNT = 1 << 16
GAMMA_SHAPES = (1.0, 2.0, 1.5, 3.5, 501.0, 4682.0, 0.3, 0.75)


def _frozen(t):
    for a in t:
        a.flags.writeable = False
    return t


@functools.lru_cache(maxsize=None)
def normal_ref(name):
    seed, site, shard, it, count = NORMAL_CASES[name]
    return _frozen(R.fill("normal", count, seed, 1.0, site, shard, it, full=True))


@functools.lru_cache(maxsize=None)
def gamma_ref(shape):
    return _frozen(R.fill("gamma", GAMMA_COUNT, GAMMA_AT["seed"], shape, GAMMA_AT["site"], GAMMA_AT["shard"],
                          GAMMA_AT["iteration"], full=True))


@functools.lru_cache(maxsize=None)
def noise_floor():
    """F_n = max |float64 NumPy Box-Muller - reference| / rad over the seed-123 counters: what the textbook
    double-precision formulation (libm log / sqrt / cos / sin of the unreduced angle 2 pi u2) loses against
    the extended-precision reference.  Measured, never hard-coded; about 6.5 u with glibc on x86-64, most
    of it the rounding of the product 2 pi u2 (an absolute angle error of up to 4 u)."""
    seed, site, shard, it, count = NORMAL_CASES["seed123"]
    ref = normal_ref("seed123")
    e = np.arange(count)
    naive = R.naive_normal_f64(seed, site, shard, e // 32, e % 32, it)
    ok = ref.rad > 0
    return float(np.max(np.abs(naive - ref.value)[ok] / ref.rad[ok]))
