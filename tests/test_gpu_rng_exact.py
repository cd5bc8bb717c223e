"""On-device Philox variates, value by value, against the extended-precision host reference
(oracle/philox_ref.py, itself pinned by tests/test_philox_ref.py).  tests/test_gpu_rng.py checks that the
variates have the right DISTRIBUTION; this file checks that each one is the documented function of its
counter: Philox4x32-10 under the full 64-bit key, the counter fields of csrc/philox.h, and log / sqrt /
sincos kernels good to a few units of roundoff.

Unit of the bars: u = 2^-53 and F_n, the error of the textbook float64 Box-Muller (libm, unreduced angle)
against the same reference, measured at the seed-123 counters (philox_cases.noise_floor; about 6.5 u).
A normal may be off by B = 2 F_n of its radius: philox.h claims "a few ulp" of the library routines, and
its sincos reduces 4u exactly where the textbook form rounds 2 pi u2, so it has no reason to be worse than
that form; the factor 2 leaves its log and sqrt a few ulp each where libm gives one.  The error is scaled
by the radius rad = sqrt(-2 log u1), not by the variate: next to a zero of the cosine a relative error says
nothing.  The gamma bounds propagate B through each formula (derived at _gamma_bound).

Limit: through dcfm_rng_fill at these counts the smallest uniform met is about 2^-23; log_u01's far
range (u down to 2^-53, products down to 2^-106) is not reached value by value here.
"""
import numpy as np
import pytest

from helpers import STATE_CMP, make_case, rel_err, state_dict
from oracle import dc_oracle as F
from philox_cases import GAMMA_AT, GAMMA_COUNT, GAMMA_SHAPES, NORMAL_CASES, R, U, gamma_ref, noise_floor, normal_ref

pytestmark = pytest.mark.gpu

MARGIN = 1e-9      # a narrower accept / reject decision may legitimately fall the other way on the device
TOL_CHAIN = 1e-10  # the project's parity bar (tests/test_gpu_parity.py)


def _normal_err(dev, ref):
    """E = max |dev - ref| / rad (a variate with rad = 0 must be exactly 0)."""
    zero = ref.rad == 0
    assert np.array_equal(dev[zero], ref.value[zero])
    return float(np.max(np.abs(dev - ref.value)[~zero] / ref.rad[~zero]))


@pytest.mark.parametrize("name", list(NORMAL_CASES))
def test_normals_match_the_reference(dcfm, name):
    seed, site, shard, it, count = NORMAL_CASES[name]
    ref = normal_ref(name)
    # what the fill exercises, known from the reference alone
    t = 4.0 * ref.u2
    q, f = np.rint(t).astype(np.int64) & 3, np.abs(t - np.rint(t))
    assert set(q.tolist()) == {0, 1, 2, 3}
    assert f.min() < 1e-4 and f.max() > 0.5 - 1e-4          # phi near 0 and near +-pi/4
    if name == "seed123":
        assert ref.u1.min() < 2.0 ** -20                     # the far tail of the log
    dev = dcfm.rng_fill("normal", count, seed=seed, site=site, shard=shard, iteration=it)
    E, Fn = _normal_err(dev, ref), noise_floor()
    print(f"normals {name}: E = {E / U:.2f} u, F_n = {Fn / U:.2f} u")
    assert E <= 2.0 * Fn, f"E = {E / U:.2f} u > 2 F_n = {2 * Fn / U:.2f} u"


BASE = dict(seed=123, site=1, shard=5, iteration=7)
ADDRESSING = (
    [dict(site=s) for s in (*range(1, 13), 15)]
    + [dict(shard=s) for s in (0, 1, 65536, 0xFFFFFF)]
    + [dict(iteration=i) for i in (0, 1, 2 ** 31 + 3)]
    + [dict(seed=124), dict(seed=123 | (0x5A5A5A5A << 32))]         # low word only, high word only
)


@pytest.mark.parametrize("change", ADDRESSING, ids=lambda c: "-".join(f"{k}{v:#x}" for k, v in c.items()))
def test_addressing_one_coordinate_at_a_time(dcfm, change):
    """4096 normals with one coordinate of (seed, site, shard, iteration) moved: the device's values are
    those of exactly that counter."""
    at = {**BASE, **change}
    dev = dcfm.rng_fill("normal", 4096, **at)
    ref = R.fill("normal", 4096, at["seed"], 1.0, at["site"], at["shard"], at["iteration"], full=True)
    assert _normal_err(dev, ref) <= 2.0 * noise_floor()


@pytest.mark.parametrize("width", [1, 7, 32, 100, 128])
def test_addressing_rows_of_any_width(dcfm, width):
    """dcfm_rng_fill_rows: variate e at row e // width, index e % width, count not a multiple of width
    (index pairs straddle nothing: an odd width's last index uses half a block)."""
    count = 4099
    dev = dcfm.rng_fill("normal", count, width=width, **BASE)
    ref = R.fill("normal", count, BASE["seed"], 1.0, BASE["site"], BASE["shard"], BASE["iteration"], width=width,
                 full=True)
    assert _normal_err(dev, ref) <= 2.0 * noise_floor()
    # gamma indices above 31 (the wide delta site reaches 127): index << 8 in the gamma counter
    devg = dcfm.rng_fill("gamma", count, shape=3.5, width=width, **BASE)
    refg = R.fill("gamma", count, BASE["seed"], 3.5, BASE["site"], BASE["shard"], BASE["iteration"], width=width,
                  full=True)
    assert refg.margin.min() >= MARGIN
    assert np.all(np.abs(devg - refg.value) <= _gamma_bound(3.5, refg))


def _mt_bound(shape, value, rad, B):
    """Marsaglia-Tsang, value = d v^3, v = 1 + c x, c = 1 / (3 sqrt d): d value / dx = 3 d c v^2 =
    sqrt(d) (value / d)^(2/3), and |delta x| <= B rad is the normal's bar; 8 u value covers the roundings of
    d and c, of 1 + c x, of the cube (two products) and of the final product."""
    d = shape - 1.0 / 3.0
    return B * rad * np.sqrt(d) * (value / d) ** (2.0 / 3.0) + 8 * U * value


def _gamma_bound(shape, ref):
    """|device - reference| allowed per variate, from the normal's bar B = 2 F_n:
      shapes 1, 2     -log(u1 [u2]): the device takes one log of the rounded product u1 u2, which moves the
                      log by up to 2 u absolute, and its log is good to B relative (the kernel the normals'
                      rad goes through: rad = sqrt(-2 log u1) within B bounds the log within 2 B);
      shape > 1       _mt_bound;
      shape < 1       value = g1 exp(log U / shape): g1's Marsaglia-Tsang bound at shape + 1, relative, plus
                      (B + 4 u)(1 + |log U| / shape): log U good to B relative moves the exponent by
                      B |log U| / shape; the quotient, exp and the last product round 4 u more."""
    B = 2.0 * noise_floor()
    v = ref.value
    if shape in (1.0, 2.0):
        return 2 * U + B * v
    if shape > 1.0:
        return _mt_bound(shape, v, ref.rad, B)
    g1 = v * np.exp(ref.abs_log_u / shape)
    return v * (_mt_bound(shape + 1.0, g1, ref.rad, B) / g1 + (B + 4 * U) * (1.0 + ref.abs_log_u / shape))


@pytest.mark.parametrize("shape", GAMMA_SHAPES)
def test_gammas_match_the_reference(dcfm, shape):
    """Every gamma of the statistical test's counters equals the reference's under _gamma_bound; since
    another attempt gives another value, the accept / reject sequence matched too.  No decision of the
    reference at these counters is narrower than MARGIN (the smallest is 2e-6), so none is left out."""
    ref = gamma_ref(shape)
    assert int(np.sum(ref.margin < MARGIN)) == 0
    dev = dcfm.rng_fill("gamma", GAMMA_COUNT, shape=shape, **GAMMA_AT)
    err, bound = np.abs(dev - ref.value), _gamma_bound(shape, ref)
    worst = int(np.argmax(err / bound))
    print(f"gamma({shape}): max |dev - ref| / ref = {np.max(err / ref.value) / U:.2f} u, "
          f"max err / bound = {err[worst] / bound[worst]:.3f} at variate {worst} (attempt {ref.attempt[worst]})")
    assert np.all(err <= bound), f"variate {worst}: |dev - ref| = {err[worst]:.3e} > {bound[worst]:.3e}"


def test_init_state_from_host_variates(dcfm):
    """dcfm_init_state against the host formula of dc:68-87 on the REFERENCE's variates at sites 7-12
    (tests/test_gpu_init.py takes them from dcfm_rng_fill).  1e-13: that test's 1e-14 arithmetic bar plus
    the variates' own few-ulp difference (a cumprod of K = 7 deltas at ~10 u each)."""
    n, P, g, K, rho, seed = 37, 19, 3, 7, 0.5, 1234
    smp = dcfm.Sampler(n, P, g, K, rho, 0, 2, 1, seed=seed)
    try:
        smp.init_state()
        got = smp.get_state()
    finally:
        smp.close()
    h = dcfm.Hyper()
    want = dcfm.initial_state(n, P, K, g, rho, h, R.PhiloxSource(seed, n, P * g, g, K, h).init())
    assert not np.any(got["Lambda"])
    for f in ("ps", "omega", "psi", "Plam", "X", "Z", "eta", "delta", "tauh"):
        assert rel_err(got[f], want[f]) < 1e-13, f


@pytest.mark.parametrize("n,p,g,K", [(20, 16, 2, 3), (40, 99, 3, 33)], ids=["K3", "K33_wide64"])
def test_generated_chain_reproduced_on_the_cpu(dcfm, n, p, g, K):
    """A generated-mode chain (every variate drawn on the device) against the CPU oracle fed the
    reference's variates at the same counters: the first check of generated mode that does not pass
    through dcfm_rng_fill."""
    seed, N = 77, 2
    c = make_case(n, p, g, K)
    smp = dcfm.Sampler(c["n"], c["P"], g, K, c["rho"], 0, N, 1, seed=seed, inject_draws=False)
    try:
        smp.set_data(c["Yd"])
        smp.set_state({f: v for f, v in state_dict(c["st"]).items() if f != "eta"})
        smp.run(1, N)
        got = smp.get_state()
        S = smp.get_sigma()
    finally:
        smp.close()
    src = R.PhiloxSource(seed, c["n"], c["p"], g, K, c["hyper"])
    ref = c["st"].copy()
    Sref = F.run_chain(c["Yd"], ref, c["rho"], c["hyper"], src.iteration, 1, N, 0, N, 1)
    for f in STATE_CMP:
        e = rel_err(got[f], getattr(ref, f))
        assert e < TOL_CHAIN, f"{f} rel err {e:.3e}"
    e = rel_err(S, Sref)
    assert e < TOL_CHAIN, f"Sigmaout rel err {e:.3e}"
